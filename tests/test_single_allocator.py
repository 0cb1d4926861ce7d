"""Device and pinned-host memory of libtrexhip has one owner (trexhip::Mem, trex_amd/csrc/mem.hip): no other file of the library calls the
HIP allocation functions, so nothing can be allocated that trexhip_destroy, free_net or trainer_free does not release.  The exceptions are
the caller-owned trexhip_device_alloc / trexhip_device_free (capi.hip), the uploader's pinned ring (upload.hip) and the exchange's probe
word (comm.hip), whose lifetimes are their own."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "trex_amd" / "csrc"
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")

# file -> the calls it may hold (a call more or less in one of these files fails too)
ALLOWED = {
    "mem.hip": {"hipMalloc": 1, "hipHostMalloc": 1, "hipFree": 2, "hipHostFree": 1},          # Mem::alloc, Mem::release, Mem::free_all
    "capi.hip": {"hipMalloc": 1, "hipFree": 1},                                               # trexhip_device_alloc / trexhip_device_free
    "upload.hip": {"hipHostMalloc": 1, "hipHostFree": 2},                                     # the pinned ring
    "comm.hip": {"hipMalloc": 1, "hipFree": 1},                                               # the probe word of trexhip_comm_*
}


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def function_of(text, pos):
    """name of the last entry point defined (at column 0) before `pos`"""
    heads = re.findall(r"^int (trexhip_\w+)\(", text[:pos], flags=re.M)
    return heads[-1] if heads else None


def test_only_the_owner_allocates():
    files = sorted(p for ext in ("*.hip", "*.h", "*.cpp") for p in CSRC.glob(ext))
    assert len(files) > 20 and (CSRC / "mem.hip") in files
    found = {}
    for p in files:
        text = strip_comments(p.read_text())
        for m in CALLS.finditer(text):
            found.setdefault(p.name, {}).setdefault(m.group(1), 0)
            found[p.name][m.group(1)] += 1
    assert found == ALLOWED, found


def test_the_calls_in_capi_are_the_caller_owned_pair():
    text = strip_comments((CSRC / "capi.hip").read_text())
    where = {m.group(1): function_of(text, m.start()) for m in CALLS.finditer(text)}
    assert where == {"hipMalloc": "trexhip_device_alloc", "hipFree": "trexhip_device_free"}, where


def test_the_context_keeps_no_capacity_beside_a_pointer():
    text = strip_comments((CSRC / "internal.h").read_text())
    ctx = text[text.index("struct trexhip_ctx {"):]
    ctx = ctx[:ctx.index("\n};")]
    assert not re.search(r"\b\w+_cap\b", ctx), re.findall(r"\b\w+_cap\b", ctx)
