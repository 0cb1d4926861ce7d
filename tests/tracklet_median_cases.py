"""Constructed stacks shared by the CPU and the GPU tests of the tracklet median."""
import numpy as np


def constructed(m):
    """uint8 [m][2][8]: per pixel a stack built to sit on an edge of the walk"""
    s = np.zeros((m, 2, 8), np.uint8)
    half = m // 2
    s[:, 0, 0] = 0                                                      # all 0
    s[:, 0, 1] = 255                                                    # all 255
    s[:half, 0, 2], s[half:, 0, 2] = 0, 255                             # half and half: 255 at an even count (the upper median), and at an odd one
    s[:half, 0, 3], s[half:, 0, 3] = 255, 0                             # the same, other order
    s[:, 0, 4] = (np.arange(m) % 256)                                   # a ramp
    s[:, 0, 5] = 0x50 + (np.arange(m) % 16)                             # one high nibble, every low one
    s[:, 0, 6] = np.where(np.arange(m) <= half, 0x30, 0x2f)             # the median is the first low nibble of its high nibble
    s[:, 0, 7] = np.where(np.arange(m) <= half, 0x3f, 0x40)             # ... and the last
    s[:, 1, 0] = np.where(np.arange(m) < half, 7, 200)                  # rank m // 2 is the first 200
    s[:, 1, 1] = np.where(np.arange(m) < half + 1, 7, 200)              # rank m // 2 is the last 7
    s[:, 1, 2:] = np.random.default_rng(m).integers(0, 256, (m, 6))
    return s
