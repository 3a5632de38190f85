"""se2gpu_map_apply_ws_bytes and se2gpu_map_apply_batch_device without a device: the exported symbols, the size of the work
space and every argument and capacity refusal, which come before the first use of the handle or of a device.  A call with
no job on a table without a point slot has nothing to erase and is SE2GPU_OK without a device; any other accepted call needs one."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_map_apply_ws_bytes", "se2gpu_map_apply_batch_device")
ARGS = ("h", "d_counts", "cap", "nframes", "d_frame_null", "d_mp_ptr", "d_obs_frame", "d_obs_ftr", "d_obs_view", "d_obs_info",
        "d_sizes_in", "m_cap", "nobs_cap", "d_job_prev", "d_job_new", "B", "d_kind", "d_src", "d_view", "d_info", "d_new_pos_w",
        "d_info_prev", "d_local_pos", "d_good_prl_row", "kinds", "d_parallax_status", "d_pos", "d_good_prl", "d_mp_null",
        "d_mp_normal", "d_ftr_mp", "d_kf_observed", "d_view_pos", "d_view_info", "d_mp_ptr_new", "d_obs_frame_new",
        "d_obs_ftr_new", "d_obs_view_new", "d_obs_info_new", "d_new_frame", "d_sizes_out", "d_job_counts", "d_ws", "ws_bytes")
BY_VALUE = dict(cap=16, nframes=4, m_cap=48, nobs_cap=256, B=2, kinds=14, ws_bytes=1 << 20)
REQUIRED = ("h", "d_counts", "d_mp_ptr", "d_obs_frame", "d_obs_ftr", "d_sizes_in", "d_job_prev", "d_job_new", "d_kind", "d_src",
            "d_view", "d_info", "d_job_counts", "d_pos", "d_good_prl", "d_mp_null", "d_mp_normal", "d_ftr_mp", "d_kf_observed",
            "d_view_pos", "d_view_info", "d_mp_ptr_new", "d_obs_frame_new", "d_obs_ftr_new", "d_new_frame", "d_sizes_out", "d_ws")
INT_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert " %s(" % name in f.read()
    assert len(capi.SYMBOLS[NAMES[1]][1]) == len(ARGS)


def test_ws_bytes():
    from se2lam_amd import capi
    w = capi.lib().se2gpu_map_apply_ws_bytes
    assert w(0, 16, 0, 0) > 0 and w(2, 16, 48, 256) % 16 == 0
    assert w(2, 16, 48, 256) >= 4 * (2 * 48 + 3 * 2 * 16 + 48 + 256)          # the claims, three row arrays, counts, sources
    assert w(3, 16, 48, 256) > w(2, 16, 48, 256) > w(2, 16, 48, 200) > w(2, 16, 40, 200)
    assert w(64, 1000, 24000, 150000) < 16 << 20                               # the measured workload: under 16 MiB
    assert [w(-1, 16, 48, 256), w(2, 0, 48, 256), w(2, 16, -1, 256), w(2, 16, 48, -1), w(65536, 16, 48, 256),
            w(65535, 16, 40000, 256)] == [-1] * 6


@pytest.fixture(scope="module")
def keep():
    """host memory the checks never follow (the handle included); 16-byte aligned for d_ws"""
    out = {}
    for k in set(ARGS) - set(BY_VALUE):
        raw = np.zeros(64 + 4, np.int32)
        out[k] = raw[(-raw.ctypes.data // 4) % 4:][:64]
        assert out[k].ctypes.data % 16 == 0
    return out


def _call(keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return capi.lib().se2gpu_map_apply_batch_device(*[b[k] for k in ARGS])


def _refused(keep, code, word, **over):
    from se2lam_amd import capi
    assert _call(keep, **over) == code, over
    assert word.encode() in capi.lib().se2gpu_last_error(), (over, capi.lib().se2gpu_last_error())


def test_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in REQUIRED:
        _refused(keep, capi.ERR_INVALID, name, **{name: None})
    for name, v in (("B", -1), ("m_cap", -1), ("nobs_cap", -1), ("cap", 0), ("nframes", 0), ("kinds", 1), ("kinds", 16), ("kinds", -2)):
        _refused(keep, capi.ERR_INVALID, name if name not in ("m_cap", "nobs_cap") else name[:-4], **{name: v})
    for name in ("d_new_pos_w", "d_info_prev", "d_local_pos", "d_good_prl_row"):
        _refused(keep, capi.ERR_INVALID, "kind 3", **{name: None})
    for name in ("d_obs_view", "d_obs_info", "d_obs_view_new", "d_obs_info_new"):
        _refused(keep, capi.ERR_INVALID, "go together", **{name: None})
    for old, new in (("d_mp_ptr", "d_mp_ptr_new"), ("d_obs_frame", "d_obs_frame_new"), ("d_obs_ftr", "d_obs_ftr_new"),
                     ("d_obs_view", "d_obs_view_new"), ("d_obs_info", "d_obs_info_new")):
        _refused(keep, capi.ERR_INVALID, "must not be the old", **{new: keep[old].ctypes.data})
    _refused(keep, capi.ERR_INVALID, "aligned", d_ws=keep["d_ws"].ctypes.data + 4)
    _refused(keep, capi.ERR_CAPACITY, "nframes * cap", nframes=1 << 16, cap=1 << 16)
    _refused(keep, capi.ERR_CAPACITY, "jobs", B=65536)
    _refused(keep, capi.ERR_CAPACITY, "jobs", B=65535, m_cap=40000)
    _refused(keep, capi.ERR_CAPACITY, "jobs", B=2, cap=1 << 20, nframes=4, nobs_cap=INT_MAX - (1 << 21))
    _refused(keep, capi.ERR_CAPACITY, "work space", ws_bytes=64)


def test_accepted_calls_need_a_device_except_the_one_with_nothing_to_do(keep):
    from se2lam_amd import capi
    assert _call(keep, B=0, m_cap=0) == capi.OK                 # no job, no point slot: nothing to erase, nothing launched
    assert _call(keep, B=0, m_cap=0, nobs_cap=0, d_obs_frame=None, d_obs_ftr=None, d_obs_frame_new=None, d_obs_ftr_new=None,
                 d_job_prev=None, d_job_new=None, d_kind=None, d_src=None, d_view=None, d_info=None, d_job_counts=None) == capi.OK
    if capi.device_count() == 0:      # (with a device these would run on the host memory of `keep`)
        assert _call(keep) == capi.ERR_NO_DEVICE
        assert _call(keep, B=0) == capi.ERR_NO_DEVICE           # a pure erase pass is work
        assert _call(keep, m_cap=0) == capi.ERR_NO_DEVICE       # and so are jobs on an empty table
        # every optional array may be missing
        assert _call(keep, d_frame_null=None, d_parallax_status=None, d_obs_view=None, d_obs_info=None, d_obs_view_new=None,
                     d_obs_info_new=None) == capi.ERR_NO_DEVICE
        assert _call(keep, kinds=6, d_new_pos_w=None, d_info_prev=None, d_local_pos=None, d_good_prl_row=None) == capi.ERR_NO_DEVICE
        assert _call(keep, kinds=0) == capi.ERR_NO_DEVICE


def test_cpp_adapter_compiles_and_runs(tmp_path):
    """include/se2lam_amd/MapUpdate.h as plain C++17 against libse2gpu: MapObservationTable and the host mirror"""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_map_apply_device")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_map_apply_device_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
