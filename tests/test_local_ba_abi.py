"""se2gpu_local_ba_batch_device, se2gpu_local_ba_ws_bytes and se2gpu_local_ba_ws_layout without a device: the exported symbols,
the work-space helpers (host only) and every argument refusal, which come before the first use of the handle or of a device;
LocalBADeviceTable of include/se2lam_amd/LocalBA.h as plain C++17."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_local_ba_batch_device", "se2gpu_local_ba_ws_bytes", "se2gpu_local_ba_ws_layout")

ARGS = ("h", "d_job_kf", "njobs", "d_win_out", "d_local_list", "d_ref_list", "kf_list_cap", "d_mp_list", "mp_list_cap", "nframes",
        "d_frame_id", "d_frame_Twb", "d_frame_Tcw", "d_frame_null", "d_odo_to", "d_odo_meas", "d_odo_cov", "d_kps_un", "d_counts",
        "cap", "d_view_pos", "level_sigma2", "nlevels", "d_pos", "m", "d_mp_ptr", "d_obs_frame", "d_obs_ftr", "nobs", "fx", "cx",
        "cy", "Tbc12", "huber_delta", "xrot_info", "z_info", "iters", "mode", "max_local", "max_ref", "max_mp", "max_obs", "d_ws",
        "d_status", "d_kf_out", "d_mp_out", "d_stats", "d_info")
BY_VALUE = dict(njobs=3, kf_list_cap=8, mp_list_cap=64, nframes=12, cap=16, nlevels=8, m=60, nobs=300, fx=500.0, cx=320.0, cy=240.0,
                huber_delta=5.99, xrot_info=1e6, z_info=1.0, iters=10, mode=0, max_local=6, max_ref=4, max_mp=60, max_obs=300)
OPTIONAL = ("d_frame_null", "d_odo_to", "d_odo_meas", "d_odo_cov", "d_stats")
REQUIRED = tuple(a for a in ARGS if a not in BY_VALUE and a not in OPTIONAL)


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
    """host memory the checks never follow (the handle included); numpy's allocations of this size are 16-byte aligned"""
    k = {a: np.zeros(64, np.float64) for a in set(ARGS) - set(BY_VALUE)}
    assert k["d_ws"].ctypes.data % 16 == 0
    return k


def _call(keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return capi.lib().se2gpu_local_ba_batch_device(*[b[k] for k in ARGS])


def _refused(keep, code, arg, **over):
    from se2lam_amd import capi
    assert _call(keep, **over) == code, over
    assert arg.encode() in capi.lib().se2gpu_last_error(), (over, capi.lib().se2gpu_last_error())


def test_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    assert len(REQUIRED) == 23
    for name in REQUIRED:
        _refused(keep, capi.ERR_INVALID, name, **{name: None})
    for name in ("d_odo_to", "d_odo_meas", "d_odo_cov"):         # together or not at all
        _refused(keep, capi.ERR_INVALID, "d_odo_to", **{name: None})
    _refused(keep, capi.ERR_INVALID, "aligned", d_ws=keep["d_ws"].ctypes.data + 8)
    for name in ("njobs", "m", "nobs"):
        _refused(keep, capi.ERR_INVALID, name, **{name: -1})
    for name in ("nframes", "cap", "kf_list_cap", "mp_list_cap", "max_local", "max_ref", "max_mp", "max_obs"):
        for v in (0, -2):
            _refused(keep, capi.ERR_INVALID, name, **{name: v})
    for iters in (0, -3, 65):
        _refused(keep, capi.ERR_INVALID, "iters", iters=iters)
    for nlevels in (0, -1, 33):
        _refused(keep, capi.ERR_INVALID, "nlevels", nlevels=nlevels)
    for mode in (2, -1):
        _refused(keep, capi.ERR_INVALID, "mode", mode=mode)
    _refused(keep, capi.ERR_CAPACITY, "nframes", nframes=4097)
    _refused(keep, capi.ERR_CAPACITY, "njobs", njobs=65536)
    _refused(keep, capi.ERR_CAPACITY, "nframes * cap", nframes=4096, cap=1 << 18)
    _refused(keep, capi.ERR_CAPACITY, "m * 3", m=1 << 30)
    _refused(keep, capi.ERR_CAPACITY, "njobs * kf_list_cap", njobs=1 << 15, kf_list_cap=1 << 16)
    _refused(keep, capi.ERR_CAPACITY, "njobs * mp_list_cap", njobs=1 << 15, mp_list_cap=1 << 16)
    _refused(keep, capi.ERR_CAPACITY, "max_mp", njobs=1 << 15, max_mp=1 << 15)
    _refused(keep, capi.ERR_CAPACITY, "max_obs", njobs=1 << 15, max_obs=1 << 15)
    _refused(keep, capi.ERR_CAPACITY, "max_local + max_ref", max_local=64, max_ref=4090)
    _refused(keep, capi.ERR_CAPACITY, "launch width", max_local=64, max_ref=2000)   # the poses alone pass 160 KiB of LDS
    _refused(keep, capi.ERR_CAPACITY, "launch width", max_local=200, max_ref=1700)
    # an illegal argument is refused before a capacity, and an empty batch launches nothing
    assert _call(keep, njobs=65536, d_ws=None) == capi.ERR_INVALID
    assert _call(keep, njobs=0) == capi.OK


def test_valid_arguments_reach_the_device_check(keep):
    from se2lam_amd import capi
    if capi.device_count() > 0:
        return                                                   # (with a device these would run on `keep`)
    assert _call(keep) == capi.ERR_NO_DEVICE
    assert _call(keep, **{k: None for k in OPTIONAL}) == capi.ERR_NO_DEVICE
    assert _call(keep, iters=1) == capi.ERR_NO_DEVICE and _call(keep, iters=64, mode=1) == capi.ERR_NO_DEVICE
    assert _call(keep, nlevels=1) == capi.ERR_NO_DEVICE and _call(keep, nlevels=32) == capi.ERR_NO_DEVICE
    assert _call(keep, m=0, nobs=0) == capi.ERR_NO_DEVICE
    assert _call(keep, nframes=4096, njobs=65535) == capi.ERR_NO_DEVICE
    assert _call(keep, max_local=50, max_ref=150) == capi.ERR_NO_DEVICE          # a window the 256- or 128-thread launch holds


def test_ws_helpers_agree_and_touch_no_device():
    from se2lam_amd import capi, localba as lb
    lib = capi.lib()
    assert len(lb.WS_ARRAYS) == 12
    for njobs, ml, mr, mm, mo in ((1, 1, 1, 1, 1), (3, 6, 4, 60, 300), (3, 2, 70, 20, 100), (256, 50, 60, 3000, 20000),
                                  (65535, 2, 1, 100, 1000)):
        PK = ml + mr
        size = dict(counts=32, fixed=PK, poses=24 * PK, o_i=4 * ml, o_j=4 * ml, o_meas=24 * ml, o_info=72 * ml, lm_ptr=4 * (mm + 1),
                    e_kf=4 * mo, e_uv=16 * mo, e_info=24 * mo, lms=24 * mm)
        nbytes, lay = lb.ws_bytes(njobs, ml, mr, mm, mo), lb.ws_layout(njobs, ml, mr, mm, mo)
        assert nbytes == lib.se2gpu_local_ba_ws_bytes(njobs, ml, mr, mm, mo) > 0
        at = 0
        for k in lb.WS_ARRAYS:
            off, stride = lay[k]
            assert off >= at and off % 16 == 0 and stride % 16 == 0 and stride >= size[k], k
            at = off + njobs * stride
        # behind them: the solver's two pairs of buffers, the controller block, desc (16 L + 44 E + 16) and ainv (6 L doubles)
        assert nbytes - at >= njobs * (2 * 24 * (PK + mm) + 16 * mm + 44 * mo + 16 + 48 * mm)
    assert lib.se2gpu_local_ba_ws_bytes(0, 1, 1, 1, 1) > 0       # an allocation of that size has an address
    off, stride = (C.c_longlong * 12)(), (C.c_longlong * 12)()
    po, ps = C.cast(off, C.c_void_p), C.cast(stride, C.c_void_p)
    for a in ((-1, 6, 4, 60, 300), (3, 0, 4, 60, 300), (3, 6, 0, 60, 300), (3, 6, 4, 0, 300), (3, 6, 4, 60, 0), (65536, 6, 4, 60, 300),
              (1 << 15, 6, 4, 1 << 15, 300), (1 << 15, 6, 4, 60, 1 << 15), (3, 64, 2000, 60, 300), (3, 64, 4090, 60, 300)):
        assert lib.se2gpu_local_ba_ws_bytes(*a) == -1, a
        assert lib.se2gpu_local_ba_ws_layout(*a, po, ps, 12) == capi.ERR_INVALID == -1
    assert lib.se2gpu_local_ba_ws_layout(3, 6, 4, 60, 300, None, ps, 12) == capi.ERR_INVALID
    assert lib.se2gpu_local_ba_ws_layout(3, 6, 4, 60, 300, po, None, 12) == capi.ERR_INVALID
    assert lib.se2gpu_local_ba_ws_layout(3, 6, 4, 60, 300, po, ps, 11) == capi.ERR_INVALID


def test_python_mirror_is_there():
    from se2lam_amd import localba as lb
    assert callable(lb.local_ba_device) and callable(lb.DeviceTables)
    assert lb.STATUS["nothing_to_optimise"] == 5


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_local_ba")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_local_ba_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
