"""se2gpu_localizer_ba_batch_device, se2gpu_localizer_ba_ws_bytes and se2gpu_localizer_ba_ws_layout without a device: the exported
symbols, the work-space helpers (host only) and every argument refusal, which come before the first use of the handle or of a
device; LocalizerDeviceTable and LocalizerBA::DoLocalBABatchDevice of include/se2lam_amd/Localizer.h as plain C++17."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_localizer_ba_batch_device", "se2gpu_localizer_ba_ws_bytes", "se2gpu_localizer_ba_ws_layout")

ARGS = ("h", "d_job_frame", "njobs", "nframes", "d_frame_Tcw", "d_frame_Twb", "d_kps_un", "d_counts", "cap", "d_ftr_mp", "d_kf_observed",
        "d_match_idx_mp", "d_pos", "m", "d_mp_null", "d_good_prl", "inv_level_sigma2", "nlevels", "fx", "cx", "cy", "Tbc12", "huber_delta",
        "xrot_info", "yrot_info", "z_info", "iters", "min_obs", "d_ws", "d_status", "d_pose_out", "d_stats", "d_info")
BY_VALUE = dict(njobs=3, nframes=6, cap=320, m=400, nlevels=8, fx=400.0, cx=320.0, cy=240.0, huber_delta=2.45, xrot_info=1e6, yrot_info=1e6,
                z_info=1.0, iters=30, min_obs=30)
OPTIONAL = ("d_frame_Twb", "d_kf_observed", "d_match_idx_mp", "d_mp_null", "d_good_prl", "d_stats")
REQUIRED = tuple(a for a in ARGS if a not in BY_VALUE and a not in OPTIONAL)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        text = f.read()
    assert " %s(" % name in text
    assert len(capi.SYMBOLS[NAMES[0]][1]) == len(ARGS)
    assert "THE njobs SLOTS OF A BATCH MUST BE PAIRWISE DISTINCT" in text and "#define SE2GPU_LOCALIZER_BA_WS_ARRAYS 8" in text


@pytest.fixture(scope="module")
def keep():
    """host memory the checks never follow (the handle included); numpy's allocations of this size are 16-byte aligned"""
    k = {a: np.zeros(64, np.float64) for a in set(ARGS) - set(BY_VALUE)}
    assert k["d_ws"].ctypes.data % 16 == 0
    return k


def _call(keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return capi.lib().se2gpu_localizer_ba_batch_device(*[b[k] for k in ARGS])


def _refused(keep, code, arg, **over):
    from se2lam_amd import capi
    assert _call(keep, **over) == code, over
    assert arg.encode() in capi.lib().se2gpu_last_error(), (over, capi.lib().se2gpu_last_error())


def test_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    assert len(REQUIRED) == 13
    for name in REQUIRED:
        _refused(keep, capi.ERR_INVALID, name, **{name: None})
    _refused(keep, capi.ERR_INVALID, "aligned", d_ws=keep["d_ws"].ctypes.data + 8)
    for name in ("njobs", "m"):
        _refused(keep, capi.ERR_INVALID, name, **{name: -1})
    for name in ("nframes", "cap"):
        for v in (0, -2):
            _refused(keep, capi.ERR_INVALID, name, **{name: v})
    for iters in (-1, 65):
        _refused(keep, capi.ERR_INVALID, "iters", iters=iters)
    for nlevels in (0, -1, 33):
        _refused(keep, capi.ERR_INVALID, "nlevels", nlevels=nlevels)
    for min_obs in (-2, -100):
        _refused(keep, capi.ERR_INVALID, "min_obs", min_obs=min_obs)
    _refused(keep, capi.ERR_CAPACITY, "njobs", njobs=65536)
    _refused(keep, capi.ERR_CAPACITY, "nframes * cap", nframes=1 << 16, cap=1 << 15)
    _refused(keep, capi.ERR_CAPACITY, "njobs * cap * 3", njobs=1 << 15, cap=1 << 15)
    _refused(keep, capi.ERR_CAPACITY, "m * 3", m=1 << 30)
    # an illegal argument is refused before a capacity, and an empty batch launches nothing
    assert _call(keep, njobs=65536, d_ws=None) == capi.ERR_INVALID
    assert _call(keep, njobs=0) == capi.OK


def test_valid_arguments_reach_the_device_check(keep):
    from se2lam_amd import capi
    if capi.device_count() > 0:
        return                                                   # (with a device these would run on `keep`)
    assert _call(keep) == capi.ERR_NO_DEVICE
    assert _call(keep, **{k: None for k in OPTIONAL}) == capi.ERR_NO_DEVICE
    assert _call(keep, iters=0) == capi.ERR_NO_DEVICE and _call(keep, iters=64) == capi.ERR_NO_DEVICE
    assert _call(keep, nlevels=1) == capi.ERR_NO_DEVICE and _call(keep, nlevels=32) == capi.ERR_NO_DEVICE
    assert _call(keep, min_obs=-1) == capi.ERR_NO_DEVICE and _call(keep, m=0) == capi.ERR_NO_DEVICE
    assert _call(keep, njobs=65535, cap=1000) == capi.ERR_NO_DEVICE


def test_ws_helpers_agree_and_touch_no_device():
    from se2lam_amd import capi, localizer as lz
    lib = capi.lib()
    assert len(lz.WS_ARRAYS) == 8
    for njobs, cap in ((1, 1), (3, 320), (5, 37), (256, 1000), (65535, 2000)):
        size = dict(counts=32, pose0=96, prior_meas=96, prior_info=288, e_ftr=4 * cap, xyz=24 * cap, uv=16 * cap, w=8 * cap)
        nbytes, lay = lz.ws_bytes(njobs, cap), lz.ws_layout(njobs, cap)
        assert nbytes == lib.se2gpu_localizer_ba_ws_bytes(njobs, cap) > 0
        at = 0
        for k in lz.WS_ARRAYS:
            off, stride = lay[k]
            assert off >= at and off % 16 == 0 and stride % 16 == 0 and stride >= size[k], k
            at = off + njobs * stride
        assert nbytes >= at
    assert lib.se2gpu_localizer_ba_ws_bytes(0, 320) > 0          # an allocation of that size has an address
    off, stride = (C.c_longlong * 8)(), (C.c_longlong * 8)()
    po, ps = C.cast(off, C.c_void_p), C.cast(stride, C.c_void_p)
    for a in ((-1, 320), (3, 0), (3, -5), (65536, 320), (1 << 15, 1 << 15)):
        assert lib.se2gpu_localizer_ba_ws_bytes(*a) == -1, a
        assert lib.se2gpu_localizer_ba_ws_layout(*a, po, ps, 8) == capi.ERR_INVALID == -1
    assert lib.se2gpu_localizer_ba_ws_layout(3, 320, None, ps, 8) == capi.ERR_INVALID
    assert lib.se2gpu_localizer_ba_ws_layout(3, 320, po, None, 8) == capi.ERR_INVALID
    assert lib.se2gpu_localizer_ba_ws_layout(3, 320, po, ps, 7) == capi.ERR_INVALID
    assert lib.se2gpu_localizer_ba_ws_layout(3, 320, po, ps, 8) == capi.OK


def test_python_mirror_is_there():
    from se2lam_amd import localizer as lz
    assert callable(lz.do_local_ba_batch_device) and callable(lz.read_gather)
    assert lz.STATUS["too_few_observations"] == 5 and lz.STATUS["non_finite"] == 6


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_localizer_ba")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_localizer_ba_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
