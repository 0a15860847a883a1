"""What a launch does before its first load (tools/entry_path.py, csrc/fastdiv.h).

* The multiply-shift and counter forms that replaced the kernels' run-time divisions equal the divisions, exhaustively: a
  stand-alone host program around the shared header (tests/entry_path_check.cpp) sweeps every dividend 0 .. 2^20 against every
  divisor 1 .. 4096, the kt0 / kt1 bounds of every nk 1 .. 360 x splits 1 .. 16, the ring-issue counters and the reduce's patch
  coordinates.  The same program built with -fsanitize=undefined,address runs a shorter dividend range.
* The freshly built gfx950 assembly of the four kernels the batch-1 pass launches most: fewer instructions in front of the
  first load than profiles/entry_path_before.txt records for the parent, no division (v_rcp_iflag) and at most one scalar wait
  on that path, no address fetched from the global offset table behind the first LDS-DMA.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stable-diffusion-1.5-lcm-onnx-rknn2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "entry_path_check.cpp")
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = [("igemm.hip", "igemm2_kernel<64, 64, 0, 4, 0, 0, 0>"), ("igemm.hip", "splitk_reduce_kernel"),
           ("conv_halo.hip", "conv_halo_pipe_kernel<8, 16, 64, 3, 0, 3, 0, 0>"), ("norm.hip", "gn_from_stats_fused_kernel")]


def host_cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def build(tmp_path, name, extra):
    cxx = host_cxx()
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-I", CSRC] + extra + ["-o", exe, SRC], capture_output=True, text=True)
    return exe, r


def test_multiply_shift_and_counters_equal_the_divisions(tmp_path):
    exe, r = build(tmp_path, "entry_path_check", [])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "20"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 4096 * (1 << 20)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The host build of the shared header, with a 2^14 dividend range (the instrumented loop is an order of magnitude slower)."""
    exe, r = build(tmp_path, "entry_path_check_san", ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("this host compiler has no sanitizer runtime: " + r.stderr[-300:])
    r = subprocess.run([exe, "14"], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-2000:]


@pytest.fixture(scope="module")
def fresh():
    import entry_path
    import load_chains
    if not load_chains.find_hipcc():
        pytest.skip("hipcc not found")
    before = entry_path.read_table(os.path.join(ROOT, "profiles", "entry_path_before.txt"))
    now = entry_path.analyze(sorted({os.path.join(CSRC, f) for f, _ in KERNELS}))
    return before, now


@pytest.mark.parametrize("src,kernel", KERNELS)
def test_path_to_the_first_load(fresh, src, kernel):
    before, now = fresh
    b, n = before[(src, kernel)], now[(src, kernel)]
    print(f"{kernel}: before {b}\n{' ' * len(kernel)}  now    {n}")
    assert n["entry"] < b["entry"], "not fewer instructions in front of the first load than the parent"
    assert n["rcp_entry"] == 0, "a run-time division in front of the first load"
    assert n["swait"] <= 1, "more than one scalar wait in front of the first load"
    assert n["got_after_dma"] == 0, "an address is fetched from the global offset table behind the first LDS-DMA"
