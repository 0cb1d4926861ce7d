"""The environment variables the library and its Python binding read are exactly those INTEGRATION.md lists, and no source under trex_amd/
still carries a dev-knob build."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def test_documented_names_are_the_names_read():
    names = set()
    for pat in ("*.hip", "*.cpp", "*.h"):
        for path in glob.glob(os.path.join(ROOT, "trex_amd", "csrc", pat)):
            names |= set(re.findall(r'getenv\(\s*"(TREXHIP_\w+)"', read(path)))
    for path in glob.glob(os.path.join(ROOT, "trex_amd", "*.py")):
        names |= set(re.findall(r'environ(?:\.get\(|\[)\s*"(TREXHIP_\w+)"', read(path)))
    section = read(os.path.join(ROOT, "INTEGRATION.md")).split("Environment variables", 1)[1].split("\n## ", 1)[0]
    listed = set(re.findall(r"^\|\s*`(TREXHIP_\w+)`", section, re.M))
    assert names and names == listed, (sorted(names - listed), sorted(listed - names))


def test_no_dev_knob_build_under_trex_amd():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "trex_amd")):
        for name in files:
            with open(os.path.join(dirpath, name), "rb") as f:
                assert b"TREXHIP_DEV_KNOBS" not in f.read(), os.path.join(dirpath, name)
