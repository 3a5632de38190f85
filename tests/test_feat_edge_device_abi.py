"""se2gpu_feat_edge_batch_device, se2gpu_feat_edge_ws_bytes and se2gpu_feat_edge_ws_layout without a device: the exported
symbols, the work-space helpers (host only) and every argument refusal, which come before the first use of the handle or of a
device; FeatEdgeDeviceTable of include/se2lam_amd/FeatEdge.h as plain C++17."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_feat_edge_batch_device", "se2gpu_feat_edge_ws_bytes", "se2gpu_feat_edge_ws_layout")

ARGS = ("h", "mode", "iters", "min_points", "huber_delta", "outlier_chi2", "Tbc12", "xrot", "yrot", "zinfo", "pair_a", "pair_b",
        "npairs", "nframes", "frame_Twc", "pos", "m", "row_cap", "pair_out", "common", "list_cap", "obs_view", "obs_info", "nobs",
        "matches", "counts", "cap", "ftr_mp", "view_pos", "view_info", "ws", "info8", "kf12_out", "z_out12", "info_out36",
        "mp_xyz_out", "outlier", "edge_chi2", "stats")
BY_VALUE = dict(mode=0, iters=15, min_points=10, huber_delta=5.99, outlier_chi2=5.0, xrot=1e6, yrot=1e6, zinfo=1.0, npairs=3, nframes=4,
                m=100, row_cap=16, list_cap=8, nobs=50, cap=16)
COMMON_PTRS = ("h", "Tbc12", "pair_a", "pair_b", "frame_Twc", "pos", "ws", "info8", "kf12_out", "z_out12", "info_out36")
COVIS_PTRS = ("pair_out", "common", "obs_view", "obs_info")
MATCH_PTRS = ("matches", "counts", "ftr_mp", "view_pos", "view_info")
OPTIONAL = ("mp_xyz_out", "outlier", "edge_chi2", "stats")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert " %s(" % name in f.read()
    assert len(capi.SYMBOLS[NAMES[0]][1]) == len(ARGS)


@pytest.fixture(scope="module")
def keep():
    """host memory the checks never follow (the handle included)"""
    return {k: np.zeros(64, np.float64) for k in set(ARGS) - set(BY_VALUE)}


def _call(keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return capi.lib().se2gpu_feat_edge_batch_device(*[b[k] for k in ARGS])


def _refused(keep, code, arg, **over):
    from se2lam_amd import capi
    assert _call(keep, **over) == code, over
    assert arg.encode() in capi.lib().se2gpu_last_error(), (over, capi.lib().se2gpu_last_error())


def test_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for mode, own, other in ((0, COVIS_PTRS, MATCH_PTRS), (1, MATCH_PTRS, COVIS_PTRS)):
        for name in COMMON_PTRS + own:
            _refused(keep, capi.ERR_INVALID, "d_" + name if name not in ("h", "Tbc12") else name, mode=mode, **{name: None})
    for mode in (2, -1):
        _refused(keep, capi.ERR_INVALID, "mode", mode=mode)
    for iters in (0, -3, 65):
        _refused(keep, capi.ERR_INVALID, "iterations", iters=iters)
    for mode in (0, 1):       # the scalars of both routes, whatever the mode
        for name in ("npairs", "m", "nobs"):
            _refused(keep, capi.ERR_INVALID, name, mode=mode, **{name: -1})
        for name in ("nframes", "cap", "row_cap", "list_cap"):
            for v in (0, -2):
                _refused(keep, capi.ERR_INVALID, name, mode=mode, **{name: v})
        _refused(keep, capi.ERR_CAPACITY, "65535", mode=mode, npairs=65536)
        _refused(keep, capi.ERR_CAPACITY, "npairs * row_cap", mode=mode, npairs=1 << 15, row_cap=1 << 15)       # 2^31
        _refused(keep, capi.ERR_CAPACITY, "nframes * cap", mode=mode, nframes=1 << 20, cap=1 << 11)
        # an illegal argument is refused before a capacity, and an empty batch launches nothing
        assert _call(keep, mode=mode, npairs=65536, ws=None) == capi.ERR_INVALID
        assert _call(keep, mode=mode, npairs=0) == capi.OK


def test_valid_arguments_reach_the_device_check(keep):
    from se2lam_amd import capi
    modes = ((0, MATCH_PTRS), (1, COVIS_PTRS)) if capi.device_count() == 0 else ()   # (with a device these would run on `keep`)
    for mode, other in modes:
        assert _call(keep, mode=mode) == capi.ERR_NO_DEVICE
        assert _call(keep, mode=mode, **{k: None for k in other + OPTIONAL}) == capi.ERR_NO_DEVICE   # the other route's arrays, the options
        assert _call(keep, mode=mode, iters=1) == capi.ERR_NO_DEVICE and _call(keep, mode=mode, iters=64) == capi.ERR_NO_DEVICE
        assert _call(keep, mode=mode, m=0, nobs=0, min_points=0) == capi.ERR_NO_DEVICE
        assert _call(keep, mode=mode, npairs=65535, row_cap=16383) == capi.ERR_NO_DEVICE                 # 2 * 65535 * 16383 < 2^31
        assert _call(keep, mode=mode, nframes=(1 << 20) - 1, cap=1 << 11) == capi.ERR_NO_DEVICE


def test_ws_helpers_agree_and_touch_no_device():
    from se2lam_amd import capi, feat_edge as fe
    lib = capi.lib()
    assert len(fe.WS_ARRAYS) == 7
    per_row = dict(count=0, kf12=0, prior_meas=0, prior_info=0, xyz=24, z=48, info=144)
    per_pair = dict(count=16, kf12=192, prior_meas=192, prior_info=576, xyz=0, z=0, info=0)
    for npairs, row_cap in ((1, 1), (1, 3), (3, 64), (3, 65), (70, 130), (256, 128), (65535, 16383)):
        nbytes, off = fe.ws_layout(npairs, row_cap)
        assert nbytes == lib.se2gpu_feat_edge_ws_bytes(npairs, row_cap) > 0
        order = [off[k] for k in fe.WS_ARRAYS]
        assert order[0] >= 0 and all(o % 8 == 0 for o in order)
        ends = [off[k] + npairs * (per_pair[k] + row_cap * per_row[k]) for k in fe.WS_ARRAYS]
        assert all(e <= s for e, s in zip(ends[:-1], order[1:])), "ascending and disjoint"
        assert ends[-1] <= nbytes
        # the scratch of the sparsifier alone (36 doubles per measurement, 144 per point) must fit behind them
        assert nbytes - ends[-1] >= npairs * row_cap * 8 * (72 + 144)
    assert lib.se2gpu_feat_edge_ws_bytes(0, 1) > 0          # an allocation of that size has an address
    for npairs, row_cap in ((-1, 8), (3, 0), (3, -1), (65536, 8), (1 << 15, 1 << 15)):
        assert lib.se2gpu_feat_edge_ws_bytes(npairs, row_cap) == -1
        off = (C.c_longlong * 7)()
        assert lib.se2gpu_feat_edge_ws_layout(npairs, row_cap, C.cast(off, C.c_void_p), 7) == capi.ERR_INVALID == -1
    off = (C.c_longlong * 7)()
    assert lib.se2gpu_feat_edge_ws_layout(3, 8, None, 7) == capi.ERR_INVALID
    assert lib.se2gpu_feat_edge_ws_layout(3, 8, C.cast(off, C.c_void_p), 6) == capi.ERR_INVALID


def test_python_mirror_is_there():
    from se2lam_amd import feat_edge as fe
    assert callable(fe.CreateFeatEdgeCovisBatchDevice) and callable(fe.CreateFeatEdgeMatchBatchDevice)


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_feat_edge_device")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_feat_edge_device_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
