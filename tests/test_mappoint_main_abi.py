"""se2gpu_mappoint_main_batch_device and se2gpu_match_projection_device without a device: the exported symbols and every
argument refusal of the batch call, which come before the first use of the handle or of a device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_mappoint_main_batch_device", "se2gpu_match_projection_device")

ARGS = ("h", "kps", "desc", "counts", "cap", "nframes", "frame_null", "view_pos", "scale_factors", "nlevels", "mp_ptr",
        "obs_frame", "obs_ftr", "m", "nobs", "prev", "info", "main_desc", "main_frame", "main_octave", "dist")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert "int %s(" % name in f.read()


@pytest.fixture(scope="module")
def valid():
    """arguments with nothing to refuse; the pointers are host memory the checks never follow (the handle included)"""
    keep = {k: np.zeros(64, np.int32) for k in ARGS if k not in ("cap", "nframes", "nlevels", "m", "nobs")}
    keep["scale_factors"] = np.ones(8, np.float32)
    a = {k: v.ctypes.data for k, v in keep.items()}
    a.update(cap=16, nframes=4, nlevels=8, m=3, nobs=5)
    return a, keep


def _call(a, **over):
    from se2lam_amd import capi
    b = dict(a)
    b.update(over)
    return capi.lib().se2gpu_mappoint_main_batch_device(*[b[k] for k in ARGS])


def test_arguments_are_refused_before_any_device_use(valid):
    from se2lam_amd import capi
    a, _ = valid
    for name in ("h", "kps", "desc", "counts", "mp_ptr", "info", "main_desc", "main_frame", "main_octave", "obs_frame", "obs_ftr"):
        assert _call(a, **{name: None}) == capi.ERR_INVALID, name
    assert _call(a, dist=None) == capi.ERR_INVALID                      # view positions need somewhere to go
    assert _call(a, scale_factors=None) == capi.ERR_INVALID             # d_view_pos without scale_factors
    for over in (dict(m=-1), dict(nobs=-1), dict(cap=0), dict(nframes=0), dict(nlevels=0)):
        assert _call(a, **over) == capi.ERR_INVALID, over
    assert _call(a, nlevels=33) == capi.ERR_CAPACITY
    assert b"32" in capi.lib().se2gpu_last_error()
    assert _call(a, nframes=1 << 20, cap=1 << 12) == capi.ERR_CAPACITY   # nframes * cap beyond 2^31 - 1
    # the optional ones may all be absent, and an empty batch is no error and needs nothing
    assert _call(a, m=0, nobs=0, frame_null=None, view_pos=None, scale_factors=None, dist=None, prev=None, obs_frame=None,
                 obs_ftr=None) == capi.OK


def test_valid_arguments_reach_the_device_check(valid):
    from se2lam_amd import capi
    a, _ = valid
    if capi.device_count() == 0:
        assert _call(a) == capi.ERR_NO_DEVICE


def test_projection_device_refuses_a_null_handle():
    from se2lam_amd import capi
    fb = capi.FrameBounds(0.0, 0.0, 640.0, 480.0)
    rc = capi.lib().se2gpu_match_projection_device(None, C.byref(fb), None, None, None, None, 0, None, 1.0, 1.0, 0.0, 0.0, None,
                                                   None, None, 0, 10, 1, 0.6, None, None)
    assert rc == capi.ERR_INVALID
