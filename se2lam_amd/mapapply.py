"""Python mirror of the map update over the C ABI (harness view; C++ twin: include/se2lam_amd/MapUpdate.h).

Reference: the bookkeeping of LocalMapper::findCorrespd (src/LocalMapper.cpp:95-168: addObservation / setViewMP / insertMP),
MapPoint::addObservation's normal vector (src/MapPoint.cpp:104-122) and the erasures of KeyFrame::setNull /
MapPoint::eraseObservation / MapPoint::setNull.  All of it happens in libse2gpu.so (se2gpu_map_apply_batch_device, HIP); the
tables stay in device memory and the calls follow one another without the host learning the sizes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import ISENT, SENT, dev_ptr as _ptr, upload as _up

ROW_FIELDS = [("job_prev", np.int32), ("job_new", np.int32), ("kind", np.uint8), ("src", np.int32), ("view", np.float32),
              ("info", np.float32), ("new_pos_w", np.float32), ("info_prev", np.float32), ("local_pos", np.float32),
              ("good_prl_row", np.uint8)]
POINT_FIELDS = [("pos", np.float32, 3), ("good_prl", np.uint8, 1), ("mp_null", np.uint8, 1), ("mp_normal", np.float32, 3)]
FEATURE_FIELDS = [("ftr_mp", np.int32, 1), ("kf_observed", np.uint8, 1), ("view_pos", np.float32, 3), ("view_info", np.float32, 9)]
TABLE_FIELDS = [("mp_ptr", np.int32, 0), ("obs_frame", np.int32, 1), ("obs_ftr", np.int32, 1), ("obs_view", np.float32, 3),
                ("obs_info", np.float32, 9)]
NSIZES = 9


def ws_bytes(B, cap, m_cap, nobs_cap) -> int:
    return int(capi.lib().se2gpu_map_apply_ws_bytes(B, cap, m_cap, nobs_cap))


def upload_rows(rows: dict) -> dict:
    """the job arrays of a batch (host arrays, B = len(job_prev)) in device memory"""
    d = {k: _up(rows[k], dt) for k, dt in ROW_FIELDS}
    d["B"] = len(rows["job_prev"])
    return d


class DeviceMap:
    """The observation table and the per-point / per-feature tables of one map in device memory, with a second CSR for the
    call to write: apply() swaps the two.  `case`: the host arrays under the names of the C ABI's arguments without d_
    (counts, frame_null, mp_ptr, obs_frame, obs_ftr, obs_view, obs_info, sizes_in, pos, good_prl, mp_null, mp_normal, ftr_mp,
    kf_observed, view_pos, view_info) and cap, m_cap, nobs_cap."""

    def __init__(self, case: dict, max_jobs: int = 0, entry_rows: bool = True, frame_null: bool = True):
        self.cap, self.nframes = int(case["cap"]), len(case["counts"])
        self.m_cap, self.nobs_cap, self.max_jobs = int(case["m_cap"]), int(case["nobs_cap"]), int(max_jobs)
        self.rows = entry_rows
        self.counts = _up(case["counts"], np.int32)
        self.frame_null = _up(case["frame_null"], np.uint8) if frame_null else None
        shape = lambda k: (self.m_cap + 1,) if k == 0 else (self.nobs_cap,) + ((k,) if k > 1 else ())
        self.old = {n: _up(case[n], dt) for n, dt, _ in TABLE_FIELDS}
        self.new = {n: _up(np.full(shape(k), ISENT if dt == np.int32 else SENT, dt), dt) for n, dt, k in TABLE_FIELDS}
        self.point = {n: _up(case[n], dt) for n, dt, _ in POINT_FIELDS}
        self.feature = {n: _up(case[n], dt) for n, dt, _ in FEATURE_FIELDS}
        sizes = np.full(NSIZES, ISENT, np.int32)
        sizes[1:3] = case["sizes_in"]
        self.sizes = _up(sizes, np.int32)                    # d_sizes_out; words 1 and 2 are the next call's d_sizes_in
        self.new_frame = _up(np.full(max(self.m_cap, 1), ISENT, np.int32), np.int32)
        self.job_counts = _up(np.full(6 * max(self.max_jobs, 1), ISENT, np.int32), np.int32)
        self.ws_bytes = ws_bytes(self.max_jobs, self.cap, self.m_cap, self.nobs_cap)
        assert self.ws_bytes > 0, "sizes the call would refuse"
        self.ws = capi.DeviceArray(self.ws_bytes)

    def apply(self, matcher, rows: dict | None = None, kinds: int = 14, parallax_status=None, sizes_in=None, swap=True) -> None:
        """se2gpu_map_apply_batch_device on `matcher`'s stream, asynchronous; rows: upload_rows() or None for an erase pass;
        parallax_status: a device array of m_cap ints or None.  sizes_in: a device pair {m_old, nobs_old} to read instead of
        the last call's sizes; swap=False leaves the old table the current one (a benchmark repeats one call that way)"""
        B = 0 if rows is None else rows["B"]
        assert B <= self.max_jobs
        r = [None] * 10 if rows is None else [_ptr(rows[k]) for k, _ in ROW_FIELDS]
        opt = lambda t, n: _ptr(t[n]) if self.rows else None
        capi.check(capi.lib().se2gpu_map_apply_batch_device(
            matcher._h, _ptr(self.counts), self.cap, self.nframes, _ptr(self.frame_null),
            _ptr(self.old["mp_ptr"]), _ptr(self.old["obs_frame"]), _ptr(self.old["obs_ftr"]), opt(self.old, "obs_view"),
            opt(self.old, "obs_info"), C.c_void_p(self.sizes.ptr.value + 4) if sizes_in is None else _ptr(sizes_in),
            self.m_cap, self.nobs_cap, r[0], r[1], B, *r[2:],
            kinds, _ptr(parallax_status), *[_ptr(self.point[n]) for n, _, _ in POINT_FIELDS],
            *[_ptr(self.feature[n]) for n, _, _ in FEATURE_FIELDS], _ptr(self.new["mp_ptr"]), _ptr(self.new["obs_frame"]),
            _ptr(self.new["obs_ftr"]), opt(self.new, "obs_view"), opt(self.new, "obs_info"), _ptr(self.new_frame),
            _ptr(self.sizes), _ptr(self.job_counts), _ptr(self.ws), self.ws_bytes))
        if swap:
            self.old, self.new = self.new, self.old

    def download(self, B: int = 0) -> dict:
        """every array the last call wrote, under the names of tests/map_apply_model.py's outputs (the caller has waited)"""
        out = {}
        for n, dt, k in POINT_FIELDS:
            out[n] = self.point[n].to_numpy(dt, (self.m_cap, k) if k > 1 else (self.m_cap,))
        nf = self.nframes * self.cap
        for n, dt, k in FEATURE_FIELDS:
            out[n] = self.feature[n].to_numpy(dt, (nf, k) if k > 1 else (nf,))
        for n, dt, k in TABLE_FIELDS:
            sh = (self.m_cap + 1,) if k == 0 else ((self.nobs_cap, k) if k > 1 else (self.nobs_cap,))
            out[n + "_new"] = self.old[n].to_numpy(dt, sh)   # after the swap
        out["new_frame"] = self.new_frame.to_numpy(np.int32, (self.m_cap,))
        out["sizes_out"] = self.sizes.to_numpy(np.int32, (NSIZES,))
        out["job_counts"] = self.job_counts.to_numpy(np.int32, (max(self.max_jobs, 1), 6))[:B]
        return out


def apply_case(matcher, case: dict) -> dict:
    """one call on a case of tests/map_apply_model.py (host arrays); waits and returns what it wrote"""
    B = len(case["job_prev"])
    dm = DeviceMap(case, max_jobs=B, entry_rows=bool(case.get("has_rows", True)), frame_null=bool(case.get("has_frame_null", True)))
    rows = upload_rows(case) if B else None
    status = _up(case["parallax_status"], np.int32) if case.get("has_status", False) else None
    dm.apply(matcher, rows, int(case["kinds"]), status)
    matcher.sync()
    return dm.download(B)
