"""Generates tests/golden/lzo1x_streams.npz: the LZO1X streams of tests/test_pv_file.py's corpus, recorded where the reference's own
minilzo is at hand (oracle/ref.mk -> oracle/_ref/libminilzo.so).  Only the streams travel, so that the tests need no reference tree.

  python tests/golden/make_lzo_fixture.py

Stored per corpus entry i:
  ref_<i>   lzo1x_1_compress(data), as pv::Frame::serialize calls it (pv.cpp:738)
  ours_<i>  this library's encoder (trexhip_lzo1x_compress) on the same data, recorded only after the reference's lzo1x_decompress
            gave the data back from it byte for byte
  sizes     len(data) per entry
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lzo_ref  # noqa: E402
from trex_amd import capi  # noqa: E402
from test_pv_file import corpus  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lzo1x_streams.npz")


def main():
    assert lzo_ref.available(), "needs the reference's minilzo (make -f oracle/ref.mk)"
    data = corpus()
    out = {"sizes": np.array([len(d) for d in data], np.int64)}
    for i, d in enumerate(data):
        ref, ours = lzo_ref.compress(d), capi.lzo1x_compress(d)
        assert bytes(lzo_ref.decompress(ref, len(d))) == d and bytes(lzo_ref.decompress(ours, len(d))) == d, i
        out["ref_%d" % i] = np.frombuffer(bytes(ref), np.uint8)
        out["ours_%d" % i] = np.frombuffer(bytes(ours), np.uint8)
    np.savez_compressed(OUT, **out)
    print("%s: %d entries, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
