"""se2gpu_mappoint_parallax_batch_device and se2gpu_kf_correspd_batch_device without a device: the exported symbols and every
argument refusal, which come before the first use of the handle or of a device."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_mappoint_parallax_batch_device", "se2gpu_kf_correspd_batch_device")

PRL = ("h", "kps_un", "counts", "cap", "nframes", "Tcw", "Twc", "P", "idkf", "mp_ptr", "obs_frame", "obs_ftr", "m", "nobs",
       "good_prl", "new_frame", "fx", "lower", "upper", "kf_observed", "status", "place", "pos", "obs_view", "obs_info")
COR = ("h", "kps_un", "counts", "cap", "nframes", "Tcw", "Twc", "P", "kf_observed", "view_pos", "job_prev", "job_new", "Tcr",
       "Trc", "matched12", "local_pos", "match_idx_mp", "B", "main_frame", "main_ftr", "main_octave", "normal", "dist", "m", "fx",
       "lower", "upper", "passes", "inv", "kind", "src", "view", "info", "new_pos_w", "info_prev", "counts_out")
BY_VALUE = dict(cap=16, nframes=4, m=3, nobs=5, B=2, fx=200.0, lower=0.3, upper=50.0, passes=7)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert "int %s(" % name in f.read()


@pytest.fixture(scope="module")
def keep():
    """host memory the checks never follow (the handle included)"""
    return {k: np.zeros(64, np.int32) for k in set(PRL + COR) - set(BY_VALUE)}


def _call(names, keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return getattr(capi.lib(), NAMES[0] if names is PRL else NAMES[1])(*[b[k] for k in names])


def test_parallax_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in ("h", "kps_un", "counts", "Tcw", "Twc", "P", "idkf", "mp_ptr", "obs_frame", "obs_ftr", "good_prl", "new_frame",
                 "status", "place", "pos", "obs_view", "obs_info"):
        assert _call(PRL, keep, **{name: None}) == capi.ERR_INVALID, name
    for over in (dict(m=-1), dict(nobs=-1), dict(cap=0), dict(nframes=0)):
        assert _call(PRL, keep, **over) == capi.ERR_INVALID, over
    assert _call(PRL, keep, nframes=1 << 20, cap=1 << 12) == capi.ERR_CAPACITY       # nframes * cap beyond 2^31 - 1
    assert _call(PRL, keep, m=0, nobs=0, obs_frame=None, obs_ftr=None, obs_view=None, obs_info=None, kf_observed=None) == capi.OK
    if capi.device_count() == 0:
        assert _call(PRL, keep) == capi.ERR_NO_DEVICE
        assert _call(PRL, keep, kf_observed=None) == capi.ERR_NO_DEVICE              # the flags are optional


def test_correspd_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in ("h", "kps_un", "counts", "Tcw", "Twc", "P", "kf_observed", "view_pos", "job_prev", "job_new", "Tcr", "Trc",
                 "matched12", "local_pos", "match_idx_mp", "main_frame", "main_ftr", "main_octave", "normal", "dist", "inv", "kind",
                 "src", "view", "info", "new_pos_w", "info_prev", "counts_out"):
        assert _call(COR, keep, **{name: None}) == capi.ERR_INVALID, name
    for over in (dict(B=-1), dict(m=-1), dict(cap=0), dict(nframes=0), dict(passes=0), dict(passes=8), dict(passes=-1)):
        assert _call(COR, keep, **over) == capi.ERR_INVALID, over
    assert _call(COR, keep, match_idx_mp=None, passes=2) == capi.ERR_INVALID
    assert b"match_idx_mp" in capi.lib().se2gpu_last_error()
    assert _call(COR, keep, nframes=1 << 20, cap=1 << 12) == capi.ERR_CAPACITY
    assert _call(COR, keep, B=1 << 20, cap=1 << 12) == capi.ERR_CAPACITY
    assert _call(COR, keep, B=0) == capi.OK
    if capi.device_count() == 0:
        assert _call(COR, keep) == capi.ERR_NO_DEVICE
        # what a pass does not read may be absent
        assert _call(COR, keep, passes=5, match_idx_mp=None, main_frame=None, main_ftr=None, main_octave=None, normal=None,
                     dist=None) == capi.ERR_NO_DEVICE
        assert _call(COR, keep, passes=1, match_idx_mp=None, local_pos=None, new_pos_w=None, info_prev=None) == capi.ERR_NO_DEVICE
        assert _call(COR, keep, passes=6, view_pos=None, Trc=None) == capi.ERR_NO_DEVICE
        assert _call(COR, keep, passes=2, m=0, main_frame=None, main_ftr=None, main_octave=None, normal=None, dist=None,
                     view_pos=None, Trc=None, local_pos=None, new_pos_w=None, info_prev=None) == capi.ERR_NO_DEVICE
