"""The identity network's launch plan (trex_amd/csrc/cnn_plan.h) on the CPU: tests/cpp/test_cnn_plan.cpp prints the plan of each case, and every
expected number below is a literal worked out by hand from the formulas the host used before the plan existed:
   conv2 passes = ceil(20 n / 3); tickets of pk = clamp(passes / (4 workgroups), 1, 16 or 32) passes; grid = min(ceil(passes / pk), workgroups),
                  workgroups = 2 CUs (two-workgroup form) or 1 CU (role split, from 3200 crops on)
   conv3 passes = ceil(100 n / 64); from 16 CUs passes on n_big3 = (7 passes / 8) / 4 tickets of 4; grid = min(n_big3 + passes - 4 n_big3, CUs)
   fc1 (ceil(n / 32), planes) or, k_fc1_split<4> above 1024 crops, (ceil(n / 128), planes); head ceil(n / 4) up to 1024 crops, else ceil(n / 16)
   re-run on the plan: conv2 4 n and conv3 bands 5 n items (any size: n tiles) on min(items, 4 CUs) workgroups
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FP32, BF16X6, BF16X3, FP16X3 = 0, 1, 2, 3


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_plan") / ("test_cnn_plan_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_plan.cpp"), "-o", path])
    return path


def plans(exe, cases):
    """cases: (W, H, CH, mode, aligned, geom, n, n_cus) -> one dict of strings per case"""
    r = subprocess.run([exe] + [",".join(str(int(v)) for v in c) for c in cases], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return [dict(kv.split("=", 1) for kv in line.split(" ")) for line in lines]


def plan(exe, n, W=80, H=80, CH=1, mode=FP16X3, aligned=True, geom=0, n_cus=256):
    return plans(exe, [(W, H, CH, mode, aligned, geom, n, n_cus)])[0]


def has(p, **want):
    got = {k: p[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}, p


def test_one_frame_of_100_crops(exe):
    has(plan(exe, 100), chain="fused_2wg", conv1="fused", conv2="512/667", pk2=1, conv3="157/157", n_big3=0, fc1="k_fc1_split<1>", fc1_grid="4,10", K=12800,
        head="k_head_small", head_grid=25, rerun=1, head_plans=1, rerun_conv1=1, conv1_grid=100, r_conv2="400/400", r_conv3="500/500", r_fc1_grid="4,10",
        r_head_grid=7)


def test_the_role_split_threshold(exe):
    has(plan(exe, 3199), chain="fused_2wg", conv2="512/21327", pk2=10)
    has(plan(exe, 3200), chain="role_split", conv1="fused", conv2="256/21334", pk2=20, conv3="256/5000", n_big3=1093, fc1="k_fc1_split<4>", fc1_grid="25,10",
        head="k_head", head_grid=200, rerun=1, head_plans=0, rerun_conv1=1, r_conv2="1024/12800", r_conv3="1024/16000", r_fc1_grid="100,10", r_head_grid=200)


def test_the_small_tail_ends_at_1024_crops(exe):
    has(plan(exe, 1024), fc1="k_fc1_split<1>", fc1_grid="32,10", head="k_head_small", head_grid=256, head_plans=1)
    has(plan(exe, 1025), fc1="k_fc1_split<4>", fc1_grid="9,10", head="k_head", head_grid=65, head_plans=0, rerun=1)


def test_conv3_tickets_start_at_16_passes_per_cu(exe):
    has(plan(exe, 2620), conv3="256/4094", n_big3=0)
    p = plan(exe, 2621)
    has(p, conv3="256/4096", n_big3=896)
    assert int(p["n_big3"]) > 0


def test_the_geometry_word(exe):
    for n in (1, 100, 3200, 12800):
        has(plan(exe, n, geom=1 << 28), chain="two_kernel", conv1="wpre", conv1_grid=n, rerun_conv1=1)
    has(plan(exe, 100, geom=1 << 28), conv2="512/667", conv3="157/157")
    has(plan(exe, 1, geom=1 << 29), chain="role_split", conv2="7/7", pk2=1)
    has(plan(exe, 12800, geom=1 << 30), chain="fused_2wg", conv2="512/85334", pk2=16)
    for bit in range(12):
        has(plan(exe, 100, geom=1 << bit), chain="fp32_act", conv1="mfma", conv2="500/500", conv3="157/157", rerun=1, rerun_conv1=0, head_plans=1)
    has(plan(exe, 3200, geom=2048 | 1 << 29), chain="fp32_act", conv3="256/5000", n_big3=0)


def test_unaligned_crops(exe):
    for n in (100, 3200):
        has(plan(exe, n, aligned=False), chain="fp32_act", conv1="valu", conv1_grid=n, rerun=1, rerun_conv1=0)
    has(plan(exe, 100, aligned=False, mode=FP32), chain="exact", conv1="valu")


def test_three_channels_never_fuse(exe):
    for n, geom in ((1, 0), (100, 0), (3200, 0), (12800, 0), (3200, 1 << 29), (100, 1 << 30)):
        has(plan(exe, n, CH=3, geom=geom), chain="two_kernel", conv1="wpre", rerun=1, rerun_conv1=1)


def test_the_exact_modes(exe):
    for mode, conv2 in ((FP32, "200/200"), (BF16X6, "400/400"), (BF16X3, "400/400")):
        has(plan(exe, 100, mode=mode), chain="exact", conv1="mfma", conv2=conv2, conv3="100/100", fc1="k_fc1", fc1_grid="4,10", K=12800, head="k_head_small",
            head_grid=25, rerun=0, head_plans=0)
        has(plan(exe, 3200, mode=mode), chain="exact", fc1="k_fc1", fc1_grid="100,10", head="k_head", head_grid=200, rerun=0)


def test_the_plane_count_never_depends_on_n(exe):
    for mode in (FP32, FP16X3):
        for n in (1, 100, 1024, 1025, 12799, 12800, 25600):
            assert plan(exe, n, mode=mode)["fc1_grid"].split(",")[1] == "10"
            assert plan(exe, n, W=100, H=60, mode=mode)["fc1_grid"].split(",")[1] == "7"


def test_any_size(exe):
    # any = conv1 tiles per crop, conv2 tiles per crop and their width in pool windows, the same of conv3
    has(plan(exe, 100, W=64, H=64), chain="any_size", conv1="any", conv1_grid=400, conv2="400/400", conv3="100/100", fc1="k_fc1", fc1_grid="4,8", K=8192,
        head="k_head", head_grid=7, rerun=1, head_plans=0, rerun_conv1=0, r_conv2="400/400", r_conv3="100/100", r_fc1_grid="4,8", r_head_grid=7, any="4,4,8,1,8")
    has(plan(exe, 3, W=100, H=60, CH=3), chain="any_size", conv1_grid=24, conv2="21/21", conv3="6/6", fc1_grid="1,7", K=10752, any="8,7,4,2,8")
    has(plan(exe, 5, W=8, H=8), chain="any_size", conv1_grid=5, conv2="5/5", conv3="5/5", fc1_grid="1,1", K=128, any="1,1,8,1,8")
    # 120x16: conv2 over 4 x 30 windows and conv3 over 2 x 15 both take the 16-wide tile (4 x 16 windows): 1 x 2 tiles and 1 x 1, 8-wide would be 4 and 2
    has(plan(exe, 33, W=120, H=16), chain="any_size", conv1_grid=132, conv2="66/66", conv3="33/33", K=3840, any="4,2,16,1,16")
    has(plan(exe, 3000, W=64, H=64), r_conv2="1024/12000", r_conv3="1024/3000", head="k_head", head_plans=0)
    has(plan(exe, 100, W=64, H=64, mode=BF16X6), chain="any_size", rerun=0, fc1="k_fc1")


def test_another_device_size(exe):
    has(plan(exe, 3200, n_cus=304), chain="role_split", conv2="304/21334", pk2=17, conv3="304/5000", n_big3=1093, r_conv2="1216/12800", r_conv3="1216/16000")
    has(plan(exe, 3199, n_cus=304), chain="fused_2wg", conv2="608/21327", pk2=8)
    has(plan(exe, 3100, n_cus=304), conv3="304/4844", n_big3=0)         # 4844 passes: tickets at 256 CUs (from 4096 on), none at 304 (from 4864 on)
    has(plan(exe, 3100, n_cus=256), conv3="256/4844", n_big3=1059)
    has(plan(exe, 100, n_cus=304), conv2="608/667", conv3="157/157", r_conv2="400/400")
