"""Python mirror of MapPoint::updateMainKFandDescriptor over the C ABI (harness view; C++ twin: include/se2lam_amd/MapPointMain.h).

Reference: src/MapPoint.cpp:228-292 - of a point's observations the one whose descriptor has the least median Hamming distance
to all of them becomes the main observation (mMainKF, mMainDescriptor, mMainOctave, mMinDist / mMaxDist); on equal medians the
first in the order of the observation container wins, so the lists are given in that order.  All compute happens in
libse2gpu.so (se2gpu_mappoint_main_batch_device, HIP); the arrays stay in device memory.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import SENTINEL_DESC, SENTINEL_DIST, SENTINEL_FRAME, SENTINEL_OCTAVE, csr, dev_ptr as _ptr, upload as up


def update_main_batch_device(matcher, d_kps, d_desc, d_counts, cap, nframes, d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs,
                             d_info, d_main_desc, d_main_frame, d_main_octave, d_dist=None, d_frame_null=None,
                             d_view_pos=None, scale_factors=None, nlevels=None, d_prev_main_frame=None):
    """se2gpu_mappoint_main_batch_device on `matcher` (an ORBmatcher): every d_* is a capi.DeviceArray or a raw device pointer,
    scale_factors a host array (nlevels defaults to its length).  Asynchronous on the matcher's stream: matcher.sync() before
    the outputs are read; matcher.match_projection_device right behind it reads d_main_desc / d_main_octave in place."""
    sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
    if nlevels is None:
        nlevels = 0 if sf is None else len(sf)
    capi.check(capi.lib().se2gpu_mappoint_main_batch_device(
        matcher._h, _ptr(d_kps), _ptr(d_desc), _ptr(d_counts), cap, nframes, _ptr(d_frame_null), _ptr(d_view_pos),
        None if sf is None else sf.ctypes.data, nlevels, _ptr(d_mp_ptr), _ptr(d_obs_frame), _ptr(d_obs_ftr), m, nobs,
        _ptr(d_prev_main_frame), _ptr(d_info), _ptr(d_main_desc), _ptr(d_main_frame), _ptr(d_main_octave), _ptr(d_dist)))


class DeviceFrames:
    """A frame set in device memory in the layout se2gpu_orb_extract_batch_device writes, uploaded from host arrays (tests,
    tools): kps (nframes * cap) capi.KP_DTYPE, desc (nframes * cap, 32) uint8, counts (nframes) int32; optional frame_null
    (nframes) uint8 and view_pos (nframes * cap, 3) float32."""

    def __init__(self, kps, desc, counts, cap, frame_null=None, view_pos=None):
        self.cap, self.nframes = int(cap), len(counts)
        self.kps, self.desc, self.counts = up(kps, capi.KP_DTYPE), up(desc, np.uint8), up(counts, np.int32)
        self.frame_null = None if frame_null is None else up(frame_null, np.uint8)
        self.view_pos = None if view_pos is None else up(view_pos, np.float32)


def sentinels(m):
    """output arrays of m points filled with values the call never writes"""
    return dict(info=np.full((m, 4), -9, np.int32), main_desc=np.full((m, 32), SENTINEL_DESC, np.uint8),
                main_frame=np.full(m, SENTINEL_FRAME, np.int32), main_octave=np.full(m, SENTINEL_OCTAVE, np.int32),
                dist=np.full((m, 2), SENTINEL_DIST, np.float32))


class MainBatch:
    """One batch on the device: the CSR lists, the previous main frames and the output arrays (initialised from `init`, default
    sentinels()).  run() launches, download() syncs and fetches."""

    def __init__(self, lists, prev_main_frame=None, init=None):
        self.m = len(lists)
        ptr, fr, ft = csr(lists)
        self.nobs = len(fr)
        self.mp_ptr, self.obs_frame, self.obs_ftr = up(ptr), up(fr), up(ft)
        self.prev = None if prev_main_frame is None else up(prev_main_frame, np.int32)
        init = init or sentinels(max(self.m, 1))
        self.out = {k: up(v) for k, v in init.items()}
        self._shapes = {k: (v.dtype, v.shape) for k, v in init.items()}

    def run(self, matcher, frames: DeviceFrames, scale_factors, with_view=True, nlevels=None):
        view = frames.view_pos if with_view else None
        update_main_batch_device(matcher, frames.kps, frames.desc, frames.counts, frames.cap, frames.nframes, self.mp_ptr,
                                 self.obs_frame, self.obs_ftr, self.m, self.nobs, self.out["info"], self.out["main_desc"],
                                 self.out["main_frame"], self.out["main_octave"], self.out["dist"], frames.frame_null, view,
                                 scale_factors, nlevels, self.prev)

    def download(self, matcher):
        matcher.sync()
        return {k: self.out[k].to_numpy(*self._shapes[k])[:self.m] for k in self.out}
