#!/usr/bin/env python3
"""Localisation: DoLocalBA for batches of frames.  se2gpu_localizer_ba_batch_device on the tables resident in device memory (renewal,
gate, gather, prior, optimize(30), pose write-back in one launch; call and one wait) against the route it replaces on the same
frames: a wait, download of the match rows, the frames' feature rows and poses and the point table, a vectorised numpy gather,
se2gpu_plane_motion_prior + se2gpu_track_pose_ba per frame, upload of the pose table.

    python tools/localizer_ba_device_bench.py [--out profiles/localizer_ba_device.json] [--md profiles/localizer_ba_device.md] [--stamp COMMIT]
    python tools/localizer_ba_device_bench.py --trace-run      # 20 device calls per batch size and nothing else: run under a kernel
                                                               # trace; the launches of k_localizer_ba tell the sizes apart by their grids

The map: 256 frame slots of cap 1000 features, 320 points of its own per frame (300 with good parallax, 10 null, 10 without), seen
from a pose 40 mm / 0.03 rad off the truth with 0.7 px of noise and 10 % outliers - the geometry of tests/test_pose_ba.py.  40 of a
frame's observations come in through the match row (the renewal), the others stand in d_ftr_mp.  1, 16 and 256 frames (distinct
slots), 30 iterations, min_obs = 30.  Both routes start every call from the same poses: the pose table is uploaded again on the
matcher's stream inside the timed span of both (12 KiB).
After two warm-up calls, windows of at least 0.3 s; medians over 7 windows with the 10th / 90th percentile.  The device's iteration
counts and final costs are compared with the host route's for every frame before anything is timed.  No figure is gated.
Not measured: counters, occupancy."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from covis_bench import stream_ms, windows  # noqa: E402
from se2lam_amd import capi, localizer as lz  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NFRAMES, CAP, PER, GOODN, RENEW, ITERS, MIN_OBS, NLEVELS = 256, 1000, 320, 300, 40, 30, 30, 8
M = NFRAMES * PER
STATS_BYTES = C.sizeof(capi.BaStats)
FX, CX, CY = 400.0, 320.0, 240.0
DELTA = float(np.sqrt(5.991))
TBC = np.eye(4)
TBC[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0.0]]
TBC[:3, 3] = [100.0, 0.0, 300.0]


def twb(x, y, th):
    c, s = np.cos(th), np.sin(th)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1.0]]
    T[:3, 3] = [x, y, 0]
    return T


def the_map(rng):
    T = dict(Tcw=np.zeros((NFRAMES, 12), np.float32), kps=np.zeros((NFRAMES, CAP), capi.KP_DTYPE), counts=np.full(NFRAMES, CAP, np.int32),
             ftr_mp=np.full((NFRAMES, CAP), -1, np.int32), kf_observed=np.zeros((NFRAMES, CAP), np.uint8), pos=np.zeros((M, 3), np.float32),
             mp_null=np.zeros(M, np.uint8), good_prl=np.ones(M, np.uint8), match=np.full((NFRAMES, CAP), -1, np.int32))
    sf = np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)
    T["inv_level_sigma2"] = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    T["kps"]["x"], T["kps"]["y"] = rng.uniform(0, 640, (NFRAMES, CAP)), rng.uniform(0, 480, (NFRAMES, CAP))
    T["kps"]["octave"] = rng.integers(0, NLEVELS, (NFRAMES, CAP))
    for f in range(NFRAMES):
        pose = np.array([rng.uniform(-2000, 2000), rng.uniform(-2000, 2000), rng.uniform(-3, 3)])
        Twc = twb(*pose) @ TBC
        start = pose + np.r_[rng.normal(0, 40, 2), rng.normal(0, 0.03)]
        T["Tcw"][f] = np.linalg.inv(twb(*start) @ TBC)[:3, :4].reshape(12)
        Xc = np.stack([rng.uniform(-2000, 2000, PER), rng.uniform(-1500, 1500, PER), rng.uniform(1500, 8000, PER)], 1)
        pts = f * PER + np.arange(PER)
        T["pos"][pts] = (Twc @ np.c_[Xc, np.ones(PER)].T).T[:, :3]
        T["mp_null"][pts[GOODN:GOODN + 10]] = 1
        T["good_prl"][pts[GOODN + 10:]] = 0
        uv = FX * Xc[:, :2] / Xc[:, 2:] + [CX, CY] + rng.normal(0, 0.7, (PER, 2))
        out = rng.random(PER) < 0.1
        uv[out] += rng.uniform(-50, 50, (int(out.sum()), 2))
        ftrs = rng.choice(CAP, PER, replace=False)
        T["kps"]["x"][f, ftrs], T["kps"]["y"][f, ftrs] = uv[:, 0], uv[:, 1]
        T["ftr_mp"][f, ftrs[RENEW:]] = pts[RENEW:]
        T["kf_observed"][f, ftrs[RENEW:]] = 1
        T["match"][f, ftrs[:RENEW]] = pts[:RENEW]                     # MatchByProjection's row: these observations are renewed
    return T


def host_gather(ftr, match, kps, pos, null, good, isig):
    """the renewal and the edges of one frame, vectorised (a row without entries out of range)"""
    ok = (match >= 0) & (match < len(null))
    ok[ok] &= null[match[ok]] == 0
    v = np.where(ok, match, ftr)
    j = np.nonzero(v >= 0)[0]
    _, last = np.unique(v[j][::-1], return_index=True)              # a point keeps its greatest feature
    j = np.sort(j[len(j) - 1 - last])
    n_obs = len(j)
    p = v[j]
    keep = (null[p] == 0) & (good[p] != 0)
    j, p = j[keep], p[keep]
    return v, n_obs, j, pos[p].astype(np.float64), np.stack([kps["x"][j], kps["y"][j]], 1).astype(np.float64), isig[kps["octave"][j]].astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--stamp", default="unknown")
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    mt = ORBmatcher()
    lib, up = capi.lib(), capi.upload
    T = the_map(np.random.default_rng(7))
    d = {k: up(T[k]) for k in ("Tcw", "kps", "counts", "ftr_mp", "kf_observed", "pos", "mp_null", "good_prl")}
    d_twb = up(np.zeros((NFRAMES, 3), np.float32))
    tbc = np.concatenate([TBC[:3, :3].reshape(-1), TBC[:3, 3]])
    K = np.array([[FX, 0, CX], [0, FX, CY], [0, 0, 1]], np.float32)
    track = C.c_void_p()
    capi.check(lib.se2gpu_track_create(C.byref(track)))
    tcw0 = np.ascontiguousarray(T["Tcw"])
    rows = []

    def down(dev, dtype, shape, offset=0):
        out = np.empty(shape, dtype)
        capi.check(lib.se2gpu_memcpy_d2h(capi.vp(out), dev.ptr.value + offset, out.nbytes))
        return out

    for J in [int(x) for x in a.sizes.split(",")]:
        jobs = np.random.default_rng(11).permutation(NFRAMES)[:J].astype(np.int32)
        d_jobs, d_match = up(jobs), up(T["match"][jobs])
        ws = capi.DeviceArray(lz.ws_bytes(J, CAP))
        d_status, d_info, d_pose = up(np.zeros(J, np.int32)), up(np.zeros((J, 8), np.int32)), up(np.zeros((J, 12)))
        d_stats = capi.DeviceArray(J * STATS_BYTES)

        def reset():
            capi.check(lib.se2gpu_memcpy_h2d_async(d["Tcw"].ptr, capi.vp(tcw0), tcw0.nbytes, mt.stream()))

        def call():
            lz.do_local_ba_batch_device(mt, d_jobs, J, NFRAMES, d["Tcw"], d_twb, d["kps"], d["counts"], CAP, d["ftr_mp"], d["kf_observed"],
                                        d_match, d["pos"], M, d["mp_null"], d["good_prl"], T["inv_level_sigma2"], K, tbc, DELTA, ws, d_status,
                                        d_pose, d_stats, d_info, iters=ITERS, min_obs=MIN_OBS)

        def device_route():
            reset()
            call()
            mt.sync()
        if a.trace_run:
            for _ in range(20):
                device_route()
            continue
        host_stats = [None] * J

        def host_route():
            reset()
            mt.sync()
            match = d_match.to_numpy(np.int32, (J, CAP))
            pos, null, good = d["pos"].to_numpy(np.float32, (M, 3)), d["mp_null"].to_numpy(np.uint8, (M,)), d["good_prl"].to_numpy(np.uint8, (M,))
            tcw = d["Tcw"].to_numpy(np.float32, (NFRAMES, 12))
            meas, info, out = np.zeros(12), np.zeros(36), np.zeros(12)
            for b, f in enumerate(jobs):
                kps = down(d["kps"], capi.KP_DTYPE, (CAP,), int(f) * CAP * capi.KP_DTYPE.itemsize)
                ftr = down(d["ftr_mp"], np.int32, (CAP,), int(f) * CAP * 4)
                v, n_obs, j, xyz, uv, w = host_gather(ftr, match[b], kps, pos, null, good, T["inv_level_sigma2"])
                if n_obs <= MIN_OBS:
                    continue
                R = tcw[f].reshape(3, 4).astype(np.float64)
                p0 = np.ascontiguousarray(np.concatenate([R[:, :3].reshape(-1), R[:, 3]]))
                capi.check(lib.se2gpu_plane_motion_prior(capi.vp(p0), capi.vp(tbc), 1e6, 1e6, 1.0, capi.vp(meas), capi.vp(info)))
                st = capi.BaStats()
                xyz, uv, w = np.ascontiguousarray(xyz), np.ascontiguousarray(uv), np.ascontiguousarray(w)
                capi.check(lib.se2gpu_track_pose_ba(track, capi.vp(p0), capi.vp(meas), capi.vp(info), len(w), capi.vp(xyz), capi.vp(uv),
                                                    capi.vp(w), FX, CX, CY, DELTA, ITERS, capi.vp(out), C.byref(st)))
                host_stats[b] = (st.iterations, st.chi2_final, len(w))
                tcw[f] = np.concatenate([out[:9].reshape(3, 3), out[9:, None]], 1).reshape(12)
            capi.check(lib.se2gpu_memcpy_h2d(d["Tcw"].ptr, capi.vp(tcw), tcw.nbytes))
        # the two routes agree
        device_route()
        status, stats, info = d_status.to_numpy(np.int32, (J,)), d_stats.to_numpy(np.uint8, (J * STATS_BYTES,)), d_info.to_numpy(np.int32, (J, 8))
        assert (status == 0).all(), status
        host_route()
        for b in range(J):
            s = capi.BaStats.from_buffer_copy(stats[b * STATS_BYTES:(b + 1) * STATS_BYTES].tobytes())
            assert host_stats[b][2] == info[b, 2] and abs(s.iterations - host_stats[b][0]) <= 12, (b, s.iterations, host_stats[b])
            assert np.isclose(s.chi2_final, host_stats[b][1], rtol=1e-6), (b, s.chi2_final, host_stats[b])
        row = {"frames": J, "edges_mean": float(info[:, 2].mean()), "observations_mean": float(info[:, 1].mean()), "renewed_mean": float(info[:, 3].mean()),
               "lm_iterations_mean": float(np.mean([capi.BaStats.from_buffer_copy(stats[b * STATS_BYTES:(b + 1) * STATS_BYTES].tobytes()).iterations
                                                    for b in range(J)])),
               "iterations": ITERS, "device_route_one_wait": windows(device_route),
               "device_call_stream_ms_per_call": stream_ms(mt, lambda: (reset(), call())), "host_route": windows(host_route)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    lib.se2gpu_track_destroy(track)
    if a.trace_run:
        return
    meta = {"commit": a.stamp, "map": {"frame_slots": NFRAMES, "cap": CAP, "points": M}, "not_measured": ["hardware counters", "occupancy"]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"_meta": meta, "localizer_ba_device": rows}, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(meta, rows))


def markdown(meta, rows):
    g = lambda r, k: "%.3f (%.3f-%.3f)" % (r[k]["median_ms"], r[k]["p10_ms"], r[k]["p90_ms"])  # noqa: E731
    cols = ("device_route_one_wait", "device_call_stream_ms_per_call", "host_route")
    out = ["# Localisation: DoLocalBA for batches of frames on the tables in device memory (tools/localizer_ba_device_bench.py)", "",
           "Commit: %s.  MI355X, one process, tables resident in device memory.  Map: %d frame slots of cap %d, %d points."
           % (meta["commit"], meta["map"]["frame_slots"], meta["map"]["cap"], meta["map"]["points"]),
           "A job = one frame: renewal from its match row, gate, gather, plane-motion prior, %d Levenberg-Marquardt iterations at most, "
           "pose write-back.  Device route: se2gpu_localizer_ba_batch_device and one wait.  Host route: a wait, download of the match rows, "
           "the frames' feature rows, the pose table and the point table, numpy gather, se2gpu_plane_motion_prior + se2gpu_track_pose_ba per "
           "frame, upload of the pose table.  Both start every call from the same poses (the pose table is uploaded inside the span)." % rows[0]["iterations"],
           "Milliseconds per batch, median (10th-90th percentile) over 7 windows of at least 0.3 s after two warm-up calls; "
           "\"on the stream\" = device events around 50 calls queued back to back, per call.", "",
           "| frames | observations, edges, renewed, LM iterations (mean) | device route, one wait | device call, on the stream | host route |",
           "|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %.0f, %.0f, %.0f, %.1f | " % (r["frames"], r["observations_mean"], r["edges_mean"], r["renewed_mean"], r["lm_iterations_mean"])
                   + " | ".join(g(r, k) for k in cols) + " |")
    out += ["", "Not measured: " + ", ".join(meta["not_measured"]) + ".", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
