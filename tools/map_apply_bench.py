#!/usr/bin/env python3
"""A new key frame's observations into the map's tables: se2gpu_map_apply_batch_device on tables resident in device memory
against the route a caller had before it - wait, download of the rows, include/se2lam_amd/MapUpdate.h's host mirror on ONE
host thread (tools/map_apply_host.cpp, g++ -O2 -ffp-contract=off), upload of the rebuilt table.

    python tools/map_apply_bench.py [--out profiles/map_apply.json]

Workload (seed 7): the map of the covisibility rows - 256 frame slots of 1,000 features, 20,000 points with 2 to 9 observations
each in frames 0..191 (about 110,000 entries), capacities 32,000 points and 200,000 entries - and 1, 16 and 64 jobs (previous
key frame b, new key frame 192 + b) of 1,000 rows with the kind mix of the reference's run (tests/golden/map_apply_ref.npz:
about 700 rows per new key frame, 110 of them new points): 450 rows of kind 1, 140 of kind 2, 110 of kind 3, 300 of kind 0.
Device: after two warm-up calls, windows of at least 0.3 s of call + se2gpu_matcher_sync (host clock), and device events
around 50 calls queued back to back; medians over 7 windows with the 10th / 90th percentile.  Every call reads the same old
table and the same sizes (swap=False, a constant d_sizes_in) and so does the same work; the in-place tables take the rows
again, which changes no count.  Host route: se2gpu_matcher_sync, blocking downloads of kind / src / view / info / new_pos_w /
info_prev and of the hasObservation table into pageable memory, the mirror, blocking uploads of the new CSR with its entry
rows (the entries in use), the per-point tables, hasObservation and mViewMPs.  The mirror alone is timed too.  The first device
call's sizes, counts and table are compared with the mirror's before anything is timed.  No figure is gated."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from se2lam_amd import capi, mapapply  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

CAP, NFRAMES, NOLD, M, M_CAP, NOBS_CAP = 1000, 256, 192, 20000, 32000, 200000
N1, N2, N3 = 450, 140, 110


def windows(fn, min_window=0.3, n_windows=7):
    fn(); fn()
    out = []
    for _ in range(n_windows):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_window:
                break
        out.append(1e3 * dt / n)
    out.sort()
    return {"median_ms": statistics.median(out), "p10_ms": out[1], "p90_ms": out[-2], "windows": len(out)}


def stream_ms(mt, fn):
    """device events around 50 calls queued back to back, per call"""
    ev, timer = [], capi.Timer()
    for _ in range(7):
        timer.start(mt.stream())
        for _ in range(50):
            fn()
        timer.stop(mt.stream())
        mt.sync()
        ev.append(timer.elapsed_ms() / 50)
    ev.sort()
    return {"median_ms": ev[3], "p10_ms": ev[1], "p90_ms": ev[5]}


def world(rng):
    """the tables of the map, at their capacities"""
    n_per = rng.integers(2, 10, M)
    ptr = np.zeros(M_CAP + 1, np.int32)
    ptr[1:M + 1] = np.cumsum(n_per)
    ptr[M + 1:] = ptr[M]
    nobs = int(ptr[M])
    frame = np.concatenate([rng.choice(NOLD, n, replace=False) for n in n_per]).astype(np.int32)
    ftr, used = np.zeros(nobs, np.int32), np.zeros(NFRAMES, np.int32)
    for i, f in enumerate(frame):              # the next free feature of the frame: a feature belongs to one point
        ftr[i] = used[f]
        used[f] += 1
    assert used.max() <= CAP - N3
    c = dict(cap=CAP, nframes=NFRAMES, m_cap=M_CAP, nobs_cap=NOBS_CAP, counts=np.full(NFRAMES, CAP, np.int32),
             frame_null=np.zeros(NFRAMES, np.uint8), mp_ptr=ptr, sizes_in=np.array([M, nobs], np.int32))
    pad = lambda a, n: np.concatenate([a, np.zeros((n - len(a),) + a.shape[1:], a.dtype)])
    c["obs_frame"], c["obs_ftr"] = pad(frame, NOBS_CAP), pad(ftr, NOBS_CAP)
    c["obs_view"] = pad(rng.normal(size=(nobs, 3)).astype(np.float32) + np.float32([0, 0, 4]), NOBS_CAP)
    c["obs_info"] = pad(rng.normal(size=(nobs, 9)).astype(np.float32), NOBS_CAP)
    c["pos"] = rng.normal(size=(M_CAP, 3)).astype(np.float32)
    c["good_prl"] = pad(rng.integers(0, 2, M).astype(np.uint8), M_CAP)
    c["mp_null"] = pad(np.zeros(M, np.uint8), M_CAP)
    c["mp_null"][M:] = 1
    c["mp_normal"] = rng.normal(size=(M_CAP, 3)).astype(np.float32)
    c["ftr_mp"] = np.full(NFRAMES * CAP, -1, np.int32)
    point = np.repeat(np.arange(M, dtype=np.int32), n_per)
    c["ftr_mp"][frame * CAP + ftr] = point
    c["kf_observed"] = (c["ftr_mp"] >= 0).astype(np.uint8)
    c["view_pos"] = rng.normal(size=(NFRAMES * CAP, 3)).astype(np.float32) + np.float32([0, 0, 4])
    c["view_info"] = rng.normal(size=(NFRAMES * CAP, 9)).astype(np.float32)
    return c, used, nobs


def jobs(c, used, B, rng):
    r = dict(job_prev=np.arange(B, dtype=np.int32), job_new=(NOLD + np.arange(B)).astype(np.int32),
             kind=np.zeros((B, CAP), np.uint8), src=np.full((B, CAP), -1, np.int32),
             view=rng.normal(size=(B, CAP, 3)).astype(np.float32) + np.float32([0, 0, 4]),
             info=rng.normal(size=(B, CAP, 9)).astype(np.float32), new_pos_w=rng.normal(size=(B, CAP, 3)).astype(np.float32),
             info_prev=rng.normal(size=(B, CAP, 9)).astype(np.float32),
             local_pos=rng.normal(size=(B, CAP, 3)).astype(np.float32) + np.float32([0, 0, 4]),
             good_prl_row=rng.integers(0, 2, (B, CAP)).astype(np.uint8))
    for b in range(B):
        held = int(used[b])
        assert held >= N1
        js = rng.permutation(CAP)[:N1 + N2 + N3]
        r["kind"][b, js[:N1]], r["src"][b, js[:N1]] = 1, rng.permutation(held)[:N1]
        seen = set(c["ftr_mp"][b * CAP:b * CAP + held].tolist())
        others = np.array([p for p in rng.permutation(M)[:4 * N2] if p not in seen][:N2], np.int32)
        r["kind"][b, js[N1:N1 + N2]], r["src"][b, js[N1:N1 + N2]] = 2, others
        r["kind"][b, js[N1 + N2:]], r["src"][b, js[N1 + N2:]] = 3, held + rng.permutation(CAP - held)[:N3]
    return r


HOST_ARGS = ["counts", "cap", "nframes", "frame_null", "mp_ptr", "obs_frame", "obs_ftr", "obs_view", "obs_info", "sizes_in", "m_cap",
             "nobs_cap", "job_prev", "job_new", "B", "kind", "src", "view", "info", "new_pos_w", "info_prev", "local_pos",
             "good_prl_row", "kinds", "parallax_status", "pos", "good_prl", "mp_null", "mp_normal", "ftr_mp", "kf_observed", "view_pos",
             "view_info", "mp_ptr_new", "obs_frame_new", "obs_ftr_new", "obs_view_new", "obs_info_new", "new_frame", "sizes_out",
             "job_counts"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,16,64")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    tmp = tempfile.mkdtemp(prefix="map_apply_")
    so = os.path.join(tmp, "libmap_apply_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "map_apply_host.cpp"), "-o", so])
    host_fn = C.CDLL(so).map_apply_host
    host_fn.restype = C.c_int
    mt = ORBmatcher()
    lib = capi.lib()
    out_rows = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(7)
        c, used, nobs = world(rng)
        r = jobs(c, used, B, rng)
        dm = mapapply.DeviceMap(c, max_jobs=B)
        rows = mapapply.upload_rows(r)
        sizes_in = capi.upload(c["sizes_in"], np.int32)
        dev = lambda: dm.apply(mt, rows, 14, None, sizes_in=sizes_in, swap=False)

        # the host's copy of everything, and the mirror on it
        h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        h.update({k: v.copy() for k, v in r.items()})
        h.update(B=B, kinds=14, parallax_status=None, mp_ptr_new=np.zeros(M_CAP + 1, np.int32), obs_frame_new=np.zeros(NOBS_CAP, np.int32),
                 obs_ftr_new=np.zeros(NOBS_CAP, np.int32), obs_view_new=np.zeros((NOBS_CAP, 3), np.float32),
                 obs_info_new=np.zeros((NOBS_CAP, 9), np.float32), new_frame=np.zeros(M_CAP, np.int32),
                 sizes_out=np.zeros(9, np.int32), job_counts=np.zeros((B, 6), np.int32))
        args = [C.c_void_p(h[k].ctypes.data) if isinstance(h[k], np.ndarray) else (None if h[k] is None else C.c_int(int(h[k])))
                for k in HOST_ARGS]
        mirror = lambda: host_fn(*args)

        # the same answer first: sizes, counts and the table
        dev()
        mt.sync()
        assert mirror() == 0
        got = dm.sizes.to_numpy(np.int32, (9,))
        assert np.array_equal(got, h["sizes_out"]), (got, h["sizes_out"])
        assert np.array_equal(dm.job_counts.to_numpy(np.int32, (B, 6)), h["job_counts"])
        n_new = int(got[2])
        for k, dt in (("mp_ptr", np.int32), ("obs_frame", np.int32), ("obs_ftr", np.int32), ("obs_view", np.float32), ("obs_info", np.float32)):
            g = dm.new[k].to_numpy(dt, h[k + "_new"].shape)
            n = M_CAP + 1 if k == "mp_ptr" else n_new
            assert np.array_equal(g[:n].view(np.uint32), h[k + "_new"][:n].view(np.uint32)), k
        assert np.array_equal(dm.point["mp_normal"].to_numpy(np.float32, (M_CAP, 3)).view(np.uint32), h["mp_normal"].view(np.uint32))

        down = [(rows[k], h[k]) for k in ("kind", "src", "view", "info", "new_pos_w", "info_prev")] + [(dm.feature["kf_observed"], h["kf_observed"])]
        m_new = int(got[1])
        up = [(dm.new["mp_ptr"], h["mp_ptr_new"]), (dm.new["obs_frame"], h["obs_frame_new"][:n_new]), (dm.new["obs_ftr"], h["obs_ftr_new"][:n_new]),
              (dm.new["obs_view"], h["obs_view_new"][:n_new]), (dm.new["obs_info"], h["obs_info_new"][:n_new]),
              (dm.point["pos"], h["pos"][:m_new]), (dm.point["good_prl"], h["good_prl"][:m_new]), (dm.point["mp_null"], h["mp_null"][:m_new]),
              (dm.point["mp_normal"], h["mp_normal"][:m_new]), (dm.feature["kf_observed"], h["kf_observed"]), (dm.feature["view_pos"], h["view_pos"])]

        def trip_down():
            mt.sync()
            for d, x in down:
                capi.check(lib.se2gpu_memcpy_d2h(capi.vp(x), d.ptr, x.nbytes))

        def trip_up():
            for d, x in up:
                capi.check(lib.se2gpu_memcpy_h2d(d.ptr, capi.vp(x), x.nbytes))

        def host_route():
            trip_down()
            mirror()
            trip_up()

        def call_and_sync():
            dev()
            mt.sync()
        row = {"jobs": B, "rows": B * CAP, "points": M, "entries": nobs, "sizes_out": got.tolist(),
               "ws_bytes": dm.ws_bytes, "bytes_down": int(sum(x.nbytes for _, x in down)), "bytes_up": int(sum(x.nbytes for _, x in up)),
               "device_call_and_sync": windows(call_and_sync), "device_stream_ms_per_call": stream_ms(mt, dev),
               "host_route": windows(host_route), "host_download": windows(trip_down), "host_mirror_one_thread": windows(mirror),
               "host_upload": windows(trip_up)}
        assert np.array_equal(dm.sizes.to_numpy(np.int32, (9,)), got), "the timed calls did not do the first call's work"
        out_rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"map_apply": out_rows}, f, indent=1)


if __name__ == "__main__":
    main()
