"""se2gpu_track_loop_verify_batch_device without a device: the exported symbols and the argument checks, the sample draw of
csrc/fm_subsets.h compiled by the host compiler against a pure-Python cv::RNG + getSubset, and the C++ mirror
(include/se2lam_amd/LoopVerify.h) as plain C++17 with its verdict helpers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("se2gpu_track_loop_verify_batch_device", "se2gpu_track_set_stream", "se2gpu_track_stream", "se2gpu_track_sync")


def test_symbols_are_exported_and_in_the_table():
    from se2lam_amd import capi
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name)


def _call(h, ptr, cap=512, nframes=4, npairs=3, has_mp=None, matches_mp=None, **nulls):
    """the entry point with `ptr` for every required pointer except those named in `nulls`"""
    from se2lam_amd import capi
    a = dict(d_kps=ptr, d_counts=ptr, d_pair_a=ptr, d_pair_b=ptr, d_matches12=ptr, d_matches_good=ptr, d_info=ptr)
    a.update(nulls)
    return capi.lib().se2gpu_track_loop_verify_batch_device(h, a["d_kps"], a["d_counts"], cap, nframes, has_mp, None, a["d_pair_a"],
                                                            a["d_pair_b"], npairs, a["d_matches12"], a["d_matches_good"],
                                                            matches_mp, a["d_info"])


def test_arguments_are_refused_before_anything_is_touched():
    """The checks come before the first use of the handle or of a device, so a stand-in address serves for both here; no call
    below gets past them."""
    from se2lam_amd import capi
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert _call(None, p) == capi.ERR_INVALID
    for name in ("d_kps", "d_counts", "d_pair_a", "d_pair_b", "d_matches12", "d_matches_good", "d_info"):
        assert _call(p, p, **{name: None}) == capi.ERR_INVALID, name
    assert _call(p, p, npairs=0) == capi.ERR_INVALID
    assert _call(p, p, cap=0) == capi.ERR_INVALID
    assert _call(p, p, nframes=0) == capi.ERR_INVALID
    assert _call(p, p, matches_mp=p) == capi.ERR_INVALID                 # d_matches_mp without d_has_mp
    assert _call(p, p, npairs=65536) == capi.ERR_CAPACITY
    assert _call(p, p, cap=65537) == capi.ERR_CAPACITY
    assert _call(p, p, has_mp=p, matches_mp=p, cap=65537) == capi.ERR_CAPACITY
    assert capi.lib().se2gpu_track_set_stream(None, None) == capi.ERR_INVALID
    assert capi.lib().se2gpu_track_sync(None) == capi.ERR_INVALID
    assert capi.lib().se2gpu_track_stream(None) is None


# ---- the sample draw --------------------------------------------------------------------------------------------------------
def _py_subsets(n, niters):
    """cv::RNG(-1) (multiply-with-carry, coefficient 4164903690) and PointSetRegistrator::getSubset: 7 distinct indices by
    rejection, one generator for the run"""
    state = (1 << 64) - 1
    out = []
    for _ in range(niters):
        idx = []
        while len(idx) < 7:
            state = ((state & 0xffffffff) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
            v = (state & 0xffffffff) % n
            if v not in idx:
                idx.append(v)
        out.append(idx)
    return out


DRAW_N = (10, 14, 15, 16, 100, 1000)


@pytest.fixture(scope="module")
def draw_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path_factory.mktemp("fm_subsets") / "cpp_fm_subsets")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp_fm_subsets.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def py_subsets():
    return {n: _py_subsets(n, 1000) for n in DRAW_N}


@pytest.mark.parametrize("serial", [0, 1], ids=["lanes", "serial_scan"])
@pytest.mark.parametrize("table_len", [0, 100], ids=["full_table", "table_of_100"])
def test_sample_draw_equals_the_python_model(draw_program, py_subsets, table_len, serial):
    """1000 samples per n: at n = 10 about 11,000 raw values, past the end of the full table as well; with 100 table values
    nearly all of every draw comes from the continued recurrence.  Both ways through a window: the scan by lanes with the
    chase over the sample starts, and the serial scan that carries a half-drawn sample from window to window."""
    r = subprocess.run([draw_program, str(table_len), "1000", str(serial)] + [str(n) for n in DRAW_N], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(DRAW_N)
    for n, line in zip(DRAW_N, lines):
        vals = [int(v) for v in line.split()]
        assert vals[0] == n
        got = [vals[1 + 7 * i:8 + 7 * i] for i in range(1000)]
        assert got == py_subsets[n], "n = %d" % n


def test_sample_draw_equals_the_oracle(draw_program, oracle):
    """the restatement the masks are held to draws the same samples (n = 15: the first RANSAC size)"""
    r = subprocess.run([draw_program, "0", "1000", "0", "15", "300"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for line in r.stdout.strip().split("\n"):
        vals = [int(v) for v in line.split()]
        assert vals[1:] == oracle.ransac_subsets(vals[0], 1000).reshape(-1).tolist()


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_loop_verify")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_loop_verify_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
