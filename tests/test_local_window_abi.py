"""se2gpu_covis_adj_words, _connect_device, _disconnect_device and se2gpu_local_window_batch_device without a device: the
exported symbols, the size of the adjacency and every argument and capacity refusal, which come before the first use of the
handle or of a device."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("se2gpu_covis_adj_words", "se2gpu_covis_connect_device", "se2gpu_covis_disconnect_device",
         "se2gpu_local_window_batch_device")

CONNECT = ("h", "adj", "nframes", "pair_a", "pair_b", "npairs", "pair_out", "flag_mask")
DISCONNECT = ("h", "adj", "nframes", "slots", "nslots")
WINDOW = ("h", "bits_kf", "bits_mp", "nframes", "m", "adj", "frame_null", "job_kf", "njobs", "search_level", "kf_order", "mp_order",
          "win_kf", "win_mp", "win_out", "local_list", "ref_list", "kf_list_cap", "mp_list", "mp_list_cap")
BY_VALUE = dict(nframes=4, m=100, npairs=3, flag_mask=1, nslots=2, njobs=2, search_level=3, kf_list_cap=4, mp_list_cap=8)
MAX_FRAMES, MAX_BLOCKS, MAX_PAIRS = 4096, (1 << 24) - 1, (1 << 31) - 256


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_in_the_table_and_in_the_header(name):
    from se2lam_amd import capi
    assert name in capi.SYMBOLS
    assert hasattr(capi.lib(), name)
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert " %s(" % name in f.read()


def test_adj_words():
    from se2lam_amd import capi
    w = capi.lib().se2gpu_covis_adj_words
    assert [w(n) for n in (1, 2, 63, 64, 65, 128, 129, 130, 256, 4096)] == [1, 2, 63, 64, 130, 256, 387, 390, 1024, 4096 * 64]
    assert w(0) == -1 and w(-5) == -1
    assert w(2 ** 31 - 1) == (2 ** 31 - 1) * 2 ** 25                   # the size is not truncated; the calls refuse it


@pytest.fixture(scope="module")
def keep():
    """host memory the checks never follow (the handle included)"""
    return {k: np.zeros(64, np.int32) for k in set(CONNECT + DISCONNECT + WINDOW) - set(BY_VALUE)}


def _call(names, keep, **over):
    from se2lam_amd import capi
    b = {k: v.ctypes.data for k, v in keep.items()}
    b.update(BY_VALUE)
    b.update(over)
    return getattr(capi.lib(), NAMES[1 + (CONNECT, DISCONNECT, WINDOW).index(names)])(*[b[k] for k in names])


def _refused(names, keep, code, arg, **over):
    from se2lam_amd import capi
    assert _call(names, keep, **over) == code, over
    assert arg.encode() in capi.lib().se2gpu_last_error(), (over, capi.lib().se2gpu_last_error())


def test_connect_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in ("h", "adj", "pair_a", "pair_b"):
        _refused(CONNECT, keep, capi.ERR_INVALID, name, **{name: None})
    for name, v in (("npairs", -1), ("nframes", 0), ("nframes", -3)):
        _refused(CONNECT, keep, capi.ERR_INVALID, name, **{name: v})
    _refused(CONNECT, keep, capi.ERR_CAPACITY, "nframes", nframes=MAX_FRAMES + 1)
    _refused(CONNECT, keep, capi.ERR_CAPACITY, "npairs", npairs=MAX_PAIRS + 1)
    assert _call(CONNECT, keep, npairs=0) == capi.OK
    assert _call(CONNECT, keep, npairs=0, pair_out=None) == capi.OK
    if capi.device_count() == 0:      # (with a device these would run on the host memory of `keep`)
        assert _call(CONNECT, keep) == capi.ERR_NO_DEVICE
        assert _call(CONNECT, keep, pair_out=None) == capi.ERR_NO_DEVICE                        # the unconditional links
        assert _call(CONNECT, keep, nframes=MAX_FRAMES, npairs=MAX_PAIRS) == capi.ERR_NO_DEVICE


def test_disconnect_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in ("h", "adj", "slots"):
        _refused(DISCONNECT, keep, capi.ERR_INVALID, name, **{name: None})
    for name, v in (("nslots", -1), ("nframes", 0)):
        _refused(DISCONNECT, keep, capi.ERR_INVALID, name, **{name: v})
    _refused(DISCONNECT, keep, capi.ERR_CAPACITY, "nframes", nframes=MAX_FRAMES + 1)
    _refused(DISCONNECT, keep, capi.ERR_CAPACITY, "nslots", nslots=MAX_BLOCKS + 1)
    assert _call(DISCONNECT, keep, nslots=0) == capi.OK
    if capi.device_count() == 0:
        assert _call(DISCONNECT, keep) == capi.ERR_NO_DEVICE
        assert _call(DISCONNECT, keep, nframes=MAX_FRAMES, nslots=MAX_BLOCKS) == capi.ERR_NO_DEVICE


def test_window_arguments_are_refused_before_any_device_use(keep):
    from se2lam_amd import capi
    for name in ("h", "bits_kf", "bits_mp", "adj", "job_kf", "win_kf", "win_mp", "win_out"):
        _refused(WINDOW, keep, capi.ERR_INVALID, name, **{name: None})
    for name, v in (("m", -1), ("njobs", -1), ("nframes", 0), ("search_level", -1), ("kf_list_cap", -1), ("mp_list_cap", -1)):
        _refused(WINDOW, keep, capi.ERR_INVALID, name, **{name: v})
    _refused(WINDOW, keep, capi.ERR_CAPACITY, "nframes", nframes=MAX_FRAMES + 1)
    _refused(WINDOW, keep, capi.ERR_CAPACITY, "d_bits", nframes=MAX_FRAMES, m=33538048 + 1)    # 4098 * 524033 words are too many
    _refused(WINDOW, keep, capi.ERR_CAPACITY, "njobs", njobs=MAX_BLOCKS + 1)
    assert _call(WINDOW, keep, njobs=0) == capi.OK
    if capi.device_count() == 0:
        assert _call(WINDOW, keep) == capi.ERR_NO_DEVICE
        # the limits admit nframes = 4096, m = 2^20 and njobs = 65535, each alone, and their own maxima
        for over in (dict(nframes=4096), dict(m=1 << 20), dict(njobs=65535), dict(nframes=MAX_FRAMES, m=33538048),
                     dict(njobs=MAX_BLOCKS), dict(m=0), dict(search_level=0), dict(search_level=2 ** 31 - 1)):
            assert _call(WINDOW, keep, **over) == capi.ERR_NO_DEVICE, over
        # every optional array may be missing
        assert _call(WINDOW, keep, frame_null=None, kf_order=None, mp_order=None, local_list=None, ref_list=None, mp_list=None,
                     kf_list_cap=0, mp_list_cap=0) == capi.ERR_NO_DEVICE
