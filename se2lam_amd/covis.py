"""Python mirror of the covisibility calls over the C ABI (harness view; C++ twin: include/se2lam_amd/Covisibility.h).

Reference: Map::compareViewMPs (src/Map.cpp:354-400, both overloads), the arithmetic behind Map::updateCovisibility (:785-799),
Map::pruneRedundantKF (:193-196), GlobalMapper::CreateFeatEdge and Localizer::UpdateCovisKFCurr.  All compute happens in
libse2gpu.so (se2gpu_covis_build_device, se2gpu_covis_pairs_device, se2gpu_covis_refset_device, HIP); the observation CSR and
the bit matrix stay in device memory.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import ISENT, SENT, dev_ptr as _ptr, upload as _up


class DeviceCovis:
    """The observation CSR of se2gpu_covis_build_device in device memory (counts: nframes ints; mp_ptr: m + 1; obs_frame /
    obs_ftr; mp_null / good_prl: m bytes or None) with the work space d_bits and d_size_obs, both starting from sentinels."""

    def __init__(self, counts, cap, mp_ptr, obs_frame, obs_ftr, mp_null=None, good_prl=None):
        self.cap, self.nframes, self.m, self.nobs = int(cap), len(counts), len(mp_ptr) - 1, len(obs_frame)
        self.counts, self.mp_ptr = _up(counts, np.int32), _up(mp_ptr, np.int32)
        self.obs_frame, self.obs_ftr = _up(obs_frame, np.int32), _up(obs_ftr, np.int32)
        self.mp_null = None if mp_null is None else _up(mp_null, np.uint8)
        self.good_prl = None if good_prl is None else _up(good_prl, np.uint8)
        self.W = (self.m + 63) // 64
        self.words = int(capi.lib().se2gpu_covis_bits_words(self.nframes, self.m))
        assert self.words == (self.nframes + 2) * self.W
        self.bits = _up(np.full(max(self.words, 1), 0xA5A5A5A5A5A5A5A5, np.uint64), np.uint64)
        self.size_obs = _up(np.full(self.nframes, ISENT, np.int32), np.int32)

    def build(self, matcher, sync=True):
        capi.check(capi.lib().se2gpu_covis_build_device(
            matcher._h, _ptr(self.counts), self.cap, self.nframes, _ptr(self.mp_ptr), _ptr(self.obs_frame), _ptr(self.obs_ftr),
            self.m, self.nobs, _ptr(self.mp_null), _ptr(self.good_prl), _ptr(self.bits), _ptr(self.size_obs)))
        if sync:
            matcher.sync()
        return self

    def read_bits(self):
        """(nframes + 2, W) uint64"""
        return self.bits.to_numpy(np.uint64, (max(self.words, 1),))[:self.words].reshape(self.nframes + 2, self.W)

    def read_size_obs(self):
        return self.size_obs.to_numpy(np.int32, (self.nframes,))


class _Pending:
    """outputs of an asynchronous call: read() after the matcher's stream was waited for"""

    def __init__(self, keep, read):
        self._keep, self.read = keep, read


def build_device(matcher, counts, cap, mp_ptr, obs_frame, obs_ftr, mp_null=None, good_prl=None) -> DeviceCovis:
    """se2gpu_covis_build_device for host arrays on `matcher`'s stream; syncs and returns the resident table."""
    return DeviceCovis(counts, cap, mp_ptr, obs_frame, obs_ftr, mp_null, good_prl).build(matcher)


def pairs_device(matcher, cv: DeviceCovis, pair_a, pair_b, ratio_f=0.3, ratio_d=0.1, list_cap=None, sync=True):
    """se2gpu_covis_pairs_device for host pair lists; list_cap None = no list.  Returns dict(out (n, 4), ratio (n, 2), common
    (n, list_cap, 3) or None); with sync=False an object whose read() gives it after matcher.sync()."""
    n = len(pair_a)
    a, b = _up(pair_a, np.int32), _up(pair_b, np.int32)
    out = _up(np.full((max(n, 1), 4), ISENT, np.int32), np.int32)
    ratio = _up(np.full((max(n, 1), 2), SENT, np.float32), np.float32)
    ncm = 0 if list_cap is None else n * list_cap
    common = None if list_cap is None else _up(np.full((max(ncm, 1), 3), ISENT, np.int32), np.int32)
    csr = [None, 0, None, None, None, 0] if list_cap is None else \
        [_ptr(cv.counts), cv.cap, _ptr(cv.mp_ptr), _ptr(cv.obs_frame), _ptr(cv.obs_ftr), cv.nobs]
    capi.check(capi.lib().se2gpu_covis_pairs_device(
        matcher._h, _ptr(cv.bits), cv.nframes, cv.m, _ptr(a), _ptr(b), n, ratio_f, ratio_d, _ptr(out), _ptr(ratio),
        _ptr(common), 0 if list_cap is None else list_cap, *csr))

    def read():
        return dict(out=out.to_numpy(np.int32, (max(n, 1), 4))[:n], ratio=ratio.to_numpy(np.float32, (max(n, 1), 2))[:n],
                    common=None if common is None else
                    common.to_numpy(np.int32, (max(ncm, 1), 3))[:ncm].reshape(n, list_cap, 3))
    if not sync:
        return _Pending((a, b, cv), read)
    matcher.sync()
    return read()


def refset_device(matcher, cv: DeviceCovis, job_kf, ref_ptr, ref_idx, k=2, thresh=0.8, sync=True):
    """se2gpu_covis_refset_device for host job lists (ref_ptr: njobs + 1).  Returns dict(out (n, 3), ratio (n,))."""
    n, nref = len(job_kf), len(ref_idx)
    kf, rp, ri = _up(job_kf, np.int32), _up(ref_ptr, np.int32), _up(ref_idx, np.int32)
    out = _up(np.full((max(n, 1), 3), ISENT, np.int32), np.int32)
    ratio = _up(np.full(max(n, 1), SENT, np.float64), np.float64)
    capi.check(capi.lib().se2gpu_covis_refset_device(matcher._h, _ptr(cv.bits), cv.nframes, cv.m, _ptr(kf), _ptr(rp), _ptr(ri),
                                                     nref, n, k, thresh, _ptr(out), _ptr(ratio)))

    def read():
        return dict(out=out.to_numpy(np.int32, (max(n, 1), 3))[:n], ratio=ratio.to_numpy(np.float64, (max(n, 1),))[:n])
    if not sync:
        return _Pending((kf, rp, ri, cv), read)
    matcher.sync()
    return read()
