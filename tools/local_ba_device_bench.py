#!/usr/bin/env python3
"""Local BA for batches of windows: se2gpu_local_window_batch_device -> se2gpu_local_ba_batch_device on the tables resident in
device memory, one wait, against the host route on the same windows (lists and tables downloaded, flattened on the host into
se2gpu_local_graph, se2gpu_ba_load_local_graph -> se2gpu_ba_initialize per window, se2gpu_ba_optimize_batch under
SE2GPU_BA_RESIDENT=1, so both routes end in the same one-workgroup-per-window solver).

    python tools/local_ba_device_bench.py [--out profiles/local_ba_device.json] [--md profiles/local_ba_device.md] [--stamp COMMIT]
    python tools/local_ba_device_bench.py --trace-run --sizes 256     # 20 device chains of 256 jobs and nothing else: run under
                                                                      # a kernel trace for the gather / solve / finish split

The map is that of tools/local_window_bench.py (seed 7: 256 key-frame slots on a ring, 20,000 points, the covisibility graph the
chain builds), given a geometry here: the slots 100 mm apart on a circle, every point 3 - 8 m ahead of its centre slot, key points
projected from the true scene with 0.5 px of noise, poses and points of the tables off by millimetres, an odometry chain.  A job is
one current key frame with search_level 3; 1, 16 and 256 jobs (distinct slots).  Timed span, device: window -> load -> optimise ->
one se2gpu_matcher_sync.  Host: window call and sync, download of the lists and of the tables the lists point into, the
flattening (numpy, vectorised: the map has no invalid entry and no frame twice in a list - checked against the general flattening
on one job first), load + initialize per window into optimizers that are kept and cleared, one optimize_batch.
After two warm-up calls, windows of at least 0.3 s; medians over 7 windows with the 10th / 90th percentile.  The device's
iteration counts and final costs are compared with the host route's for every job before anything is timed.  No figure is gated.
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

from covis_bench import CAP, M, NFRAMES, nearest, stream_ms, the_map, windows  # noqa: E402
from se2lam_amd import capi, covis, localba as lb, localwindow as lw, optimizer as op  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NNEAR, LEVEL, ITERS = 12, 3, 10
STATS_BYTES = C.sizeof(capi.BaStats)
FX, CX, CY = 520.0, 320.0, 240.0
RBC = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
TBC = np.array([100.0, 0.0, 300.0])


def tcw(twb):
    x, y, th = twb
    c, s = np.cos(th), np.sin(th)
    Twb = np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, 0], [0, 0, 0, 1]])
    Tbc = np.eye(4)
    Tbc[:3, :3], Tbc[:3, 3] = RBC, TBC
    return (np.linalg.inv(Tbc) @ np.linalg.inv(Twb))[:3]


def geometry(mp, rng):
    """the tables of se2gpu_local_ba_batch_device for the_map's topology"""
    radius = 100.0 * NFRAMES / (2 * np.pi)
    ang = 2 * np.pi * np.arange(NFRAMES) / NFRAMES
    head = (ang + np.pi / 2 + np.pi) % (2 * np.pi) - np.pi
    truth = np.c_[radius * np.cos(ang), radius * np.sin(ang), head]
    Twb = (truth + np.c_[rng.normal(0, 5, (NFRAMES, 2)), rng.normal(0, 0.002, NFRAMES)]).astype(np.float32)
    Tcw_true = np.stack([tcw(t) for t in truth])
    Tcw = np.stack([tcw(t.astype(np.float64)) for t in Twb]).astype(np.float32)
    ptr, of, ok = mp["ptr"], mp["obs_frame"], mp["obs_ftr"]
    centre = np.array([int(np.round(np.angle(np.exp(1j * ang[of[ptr[p]:ptr[p + 1]]]).sum()) / (2 * np.pi) * NFRAMES)) % NFRAMES
                       for p in range(M)])
    body = np.c_[rng.uniform(3000, 8000, M), rng.uniform(-2000, 2000, M), rng.uniform(0, 2500, M)]
    c, s = np.cos(truth[centre, 2]), np.sin(truth[centre, 2])
    world = np.c_[truth[centre, 0] + c * body[:, 0] - s * body[:, 1], truth[centre, 1] + s * body[:, 0] + c * body[:, 1], body[:, 2]]
    pos = (world + rng.normal(0, 20, (M, 3))).astype(np.float32)
    owner = np.repeat(np.arange(M), np.diff(ptr))
    lc_true = np.einsum("nij,nj->ni", Tcw_true[of][:, :, :3], world[owner]) + Tcw_true[of][:, :, 3]
    assert (lc_true[:, 2] > 500).all(), "a point behind or at a camera"
    kps = np.zeros((NFRAMES, CAP), capi.KP_DTYPE)
    uv = FX * lc_true[:, :2] / lc_true[:, 2:3] + np.array([CX, CY]) + rng.normal(0, 0.5, (len(of), 2))
    kps["x"][of, ok], kps["y"][of, ok] = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    kps["octave"][of, ok] = rng.integers(0, 8, len(of))
    view_pos = np.zeros((NFRAMES, CAP, 3), np.float32)
    view_pos[..., 2] = 1000
    view_pos[of, ok] = (np.einsum("nij,nj->ni", Tcw[of][:, :, :3].astype(np.float64), pos[owner].astype(np.float64))
                        + Tcw[of][:, :, 3]).astype(np.float32)
    nxt = (np.arange(NFRAMES) + 1) % NFRAMES
    d = truth[nxt, :2] - truth[:, :2]
    c, s = np.cos(truth[:, 2]), np.sin(truth[:, 2])
    dth = (truth[nxt, 2] - truth[:, 2] + np.pi) % (2 * np.pi) - np.pi
    odo_meas = np.c_[c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], dth]
    odo_to = nxt.astype(np.int32)
    odo_to[np.abs(truth[nxt, 2] - truth[:, 2]) > 1] = -1        # no edge across the +-pi seam: PreEdgeSE2 has no angle wrap
    odo_cov = np.tile(np.diag([25.0, 25.0, 1e-5]).reshape(-1), (NFRAMES, 1))
    return dict(frame_id=np.arange(NFRAMES, dtype=np.int32) + 2, Twb=Twb, Tcw=Tcw.reshape(NFRAMES, 12), frame_null=None, odo_to=odo_to,
                odo_meas=odo_meas, odo_cov=odo_cov, kps=kps, kps_xy=np.stack([kps["x"], kps["y"]], axis=-1), kps_octave=kps["octave"],
                counts=mp["counts"], cap=CAP, view_pos=view_pos, level_sigma2=(np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2,
                pos=pos, mp_ptr=ptr, obs_frame=of, obs_ftr=ok, K=np.array([[FX, 0, CX], [0, FX, CY], [0, 0, 1]], np.float32),
                Tbc12=np.r_[RBC.reshape(-1), TBC], huber=float(np.float32(np.sqrt(5.991))), xrot_info=1e6, z_info=1.0)


def flatten_fast(T, local, ref, mps):
    """lb.flatten_local_graph for a map without invalid entries, null key frames, frames twice in a list or octaves out of range"""
    slots = np.r_[local, ref].astype(np.int64)
    nl = len(local)
    vertex = np.full(NFRAMES, -1, np.int64)
    vertex[slots] = np.arange(len(slots))
    t = T["odo_to"][local]
    tv = np.where(t >= 0, vertex[np.maximum(t, 0)], -1)
    odo_to = np.where((tv >= 0) & (tv < nl), tv, -1).astype(np.int32)
    s, e = T["mp_ptr"][mps], T["mp_ptr"][np.asarray(mps) + 1]
    n = e - s
    idx = np.repeat(s - np.r_[0, np.cumsum(n)[:-1]], n) + np.arange(int(n.sum()))
    f, k, owner = T["obs_frame"][idx], T["obs_ftr"][idx], np.repeat(np.arange(len(mps)), n)
    keep = vertex[f] >= 0
    f, k, owner = f[keep], k[keep], owner[keep]
    Tcw = T["Tcw"].reshape(NFRAMES, 3, 4)
    return dict(kf_id=T["frame_id"][slots], kf_Twb=T["Twb"][slots], kf_Rcw=Tcw[slots][:, :, :3].reshape(-1, 9), n_local=nl, odo_to=odo_to,
                odo_meas=np.where(odo_to[:, None] >= 0, T["odo_meas"][local], 0.0),
                odo_cov=np.where(odo_to[:, None] >= 0, T["odo_cov"][local], np.eye(3).reshape(-1)), mp_pos=T["pos"][mps], obs_mp=owner.astype(np.int32),
                obs_kf=vertex[f].astype(np.int32), obs_uv=T["kps_xy"][f, k], obs_lc=T["view_pos"][f, k],
                obs_sigma2=T["level_sigma2"][T["kps_octave"][f, k]], K=T["K"], Rbc=T["Tbc12"][:9].reshape(3, 3), tbc=T["Tbc12"][9:],
                huber=T["huber"], xrot_info=T["xrot_info"], z_info=T["z_info"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--stamp", default="unknown")
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    os.environ["SE2GPU_BA_RESIDENT"] = "1"
    mt = ORBmatcher()
    lib, up = capi.lib(), capi.upload
    mp = the_map(np.random.default_rng(7))
    T = geometry(mp, np.random.default_rng(8))
    cv = covis.DeviceCovis(mp["counts"], CAP, mp["ptr"], mp["obs_frame"], mp["obs_ftr"], mp["null"], mp["good"])
    pa = np.repeat(np.arange(NFRAMES, dtype=np.int32), NNEAR)
    pb = np.concatenate([nearest(f, NNEAR) for f in range(NFRAMES)]).astype(np.int32)
    d_a, d_b = up(pa, np.int32), up(pb, np.int32)
    d_pout, d_prat = up(np.zeros((len(pa), 4)), np.int32), up(np.zeros((len(pa), 2)), np.float32)
    adj = lw.DeviceAdjacency(NFRAMES)
    cv.build(mt, sync=False)
    capi.check(lib.se2gpu_covis_pairs_device(mt._h, cv.bits.ptr, NFRAMES, M, d_a.ptr, d_b.ptr, len(pa), 0.3, 0.1, d_pout.ptr, d_prat.ptr,
                                             None, 0, None, 0, None, None, None, 0))
    capi.check(lib.se2gpu_covis_connect_device(mt._h, adj.adj.ptr, NFRAMES, d_a.ptr, d_b.ptr, len(pa), d_pout.ptr, 1))
    mt.sync()
    dT = lb.DeviceTables(T["frame_id"], T["Twb"], T["Tcw"], T["kps"], T["counts"], T["view_pos"], T["level_sigma2"], T["pos"], T["mp_ptr"],
                         T["obs_frame"], T["obs_ftr"], odo_to=T["odo_to"], odo_meas=T["odo_meas"], odo_cov=T["odo_cov"])
    W, WF = cv.W, adj.WF
    tbc = np.ascontiguousarray(T["Tbc12"], np.float64)
    rows = []
    for J in [int(x) for x in a.sizes.split(",")][:1 if a.trace_run else None]:
        jobs = np.random.default_rng(11).permutation(NFRAMES)[:J].astype(np.int32)
        d_jobs = up(jobs, np.int32)
        d_wkf, d_wmp = up(np.zeros(J * 2 * WF, np.uint64), np.uint64), up(np.zeros(J * W, np.uint64), np.uint64)
        d_out = up(np.zeros((J, 4)), np.int32)
        d_ll, d_rl, d_ml = up(np.zeros(J * NFRAMES), np.int32), up(np.zeros(J * NFRAMES), np.int32), up(np.zeros(J * M), np.int32)

        def window():
            capi.check(lib.se2gpu_local_window_batch_device(mt._h, cv.bits.ptr, cv.bits.ptr, NFRAMES, M, adj.adj.ptr, None, d_jobs.ptr,
                                                            J, LEVEL, None, None, d_wkf.ptr, d_wmp.ptr, d_out.ptr, d_ll.ptr, d_rl.ptr,
                                                            NFRAMES, d_ml.ptr, M))
        window()
        mt.sync()
        out = d_out.to_numpy(np.int32, (J, 4))
        ml_, mr_, mm_, mo_ = (int(out[:, k].max()) for k in range(4))
        PK = ml_ + mr_
        ws = capi.DeviceArray(lb.ws_bytes(J, ml_, mr_, mm_, mo_))
        d_status, d_info = up(np.zeros(J), np.int32), up(np.zeros((J, 8)), np.int32)
        d_kf, d_mpo = up(np.zeros((J, PK, 3))), up(np.zeros((J, mm_, 3)))
        d_stats = capi.DeviceArray(J * STATS_BYTES)

        def local_ba():
            capi.check(lib.se2gpu_local_ba_batch_device(
                mt._h, d_jobs.ptr, J, d_out.ptr, d_ll.ptr, d_rl.ptr, NFRAMES, d_ml.ptr, M, NFRAMES, dT.frame_id.ptr, dT.Twb.ptr, dT.Tcw.ptr,
                None, dT.odo_to.ptr, dT.odo_meas.ptr, dT.odo_cov.ptr, dT.kps.ptr, dT.counts.ptr, CAP, dT.view_pos.ptr,
                capi.vp(dT.level_sigma2), 8, dT.pos.ptr, M, dT.mp_ptr.ptr, dT.obs_frame.ptr, dT.obs_ftr.ptr, dT.nobs, FX, CX, CY, capi.vp(tbc),
                T["huber"], 1e6, 1.0, ITERS, 0, ml_, mr_, mm_, mo_, ws.ptr, d_status.ptr, d_kf.ptr, d_mpo.ptr, d_stats.ptr, d_info.ptr))

        def device_route():
            window()
            local_ba()
            mt.sync()
        if a.trace_run:
            for _ in range(20):
                device_route()
            return
        opts = [op.SlamOptimizer() for _ in range(J)]
        TABLES = (("frame_id", np.int32, (NFRAMES,)), ("Twb", np.float32, (NFRAMES, 3)), ("Tcw", np.float32, (NFRAMES, 12)),
                  ("odo_to", np.int32, (NFRAMES,)), ("odo_meas", np.float64, (NFRAMES, 3)), ("odo_cov", np.float64, (NFRAMES, 9)),
                  ("counts", np.int32, (NFRAMES,)), ("view_pos", np.float32, (NFRAMES, CAP, 3)), ("pos", np.float32, (M, 3)),
                  ("mp_ptr", np.int32, (M + 1,)), ("obs_frame", np.int32, (dT.nobs,)), ("obs_ftr", np.int32, (dT.nobs,)))

        def host_route(flatten=flatten_fast):
            window()
            mt.sync()
            o4 = d_out.to_numpy(np.int32, (J, 4))
            ll, rl = d_ll.to_numpy(np.int32, (J, NFRAMES)), d_rl.to_numpy(np.int32, (J, NFRAMES))
            ml = d_ml.to_numpy(np.int32, (J, M))
            H = dict(T)                                          # the configuration; the tables come down from the device
            for name, dtype, shape in TABLES:
                H[name] = getattr(dT, name).to_numpy(dtype, shape)
            k = dT.kps.to_numpy(capi.KP_DTYPE, (NFRAMES, CAP))
            H["kps_xy"], H["kps_octave"] = np.stack([k["x"], k["y"]], axis=-1), k["octave"]
            for j, o in enumerate(opts):
                o.clear()
                op.loadLocalGraph(o, **flatten(H, ll[j, :o4[j, 0]], rl[j, :o4[j, 1]], ml[j, :o4[j, 2]]))
                o.initializeOptimization(0)
            op.optimize_batch(opts, ITERS)
        # the two routes agree, and the fast flattening is the general one on this map
        device_route()
        status, stats = d_status.to_numpy(np.int32, (J,)), d_stats.to_numpy(np.uint8, (J * STATS_BYTES,))
        assert (status == 0).all(), status
        host_route()
        assert capi.lib().se2gpu_ba_last_batch_path() == 2
        for j, o in enumerate(opts):
            s = capi.BaStats.from_buffer_copy(stats[j * STATS_BYTES:(j + 1) * STATS_BYTES].tobytes())
            assert s.iterations == o.stats["iterations"] and np.isclose(s.chi2_final, o.stats["chi2_final"], rtol=1e-6), (j, s.chi2_final)
        ll, rl, ml = d_ll.to_numpy(np.int32, (J, NFRAMES)), d_rl.to_numpy(np.int32, (J, NFRAMES)), d_ml.to_numpy(np.int32, (J, M))
        fa = flatten_fast(T, ll[0, :out[0, 0]], rl[0, :out[0, 1]], ml[0, :out[0, 2]])
        fb = lb.flatten_local_graph(T, ll[0, :out[0, 0]], rl[0, :out[0, 1]], ml[0, :out[0, 2]])
        assert all(np.array_equal(np.asarray(fa[k]), np.asarray(fb[k])) for k in fa), "the fast flattening differs"
        info = d_info.to_numpy(np.int32, (J, 8))
        row = {"jobs": J, "local_kfs_mean": float(out[:, 0].mean()), "ref_kfs_mean": float(out[:, 1].mean()),
               "points_mean": float(out[:, 2].mean()), "edges_mean": float(info[:, 3].mean()), "free_kfs_mean": float(info[:, 1].mean()),
               "caps": [ml_, mr_, mm_, mo_], "iterations": ITERS,
               "device_route_one_wait": windows(device_route), "device_route_stream_ms_per_call": stream_ms(mt, lambda: (window(), local_ba())),
               "local_ba_stream_ms_per_call": stream_ms(mt, local_ba), "window_stream_ms_per_call": stream_ms(mt, window),
               "host_route": windows(host_route)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del opts
    meta = {"commit": a.stamp, "map": {"key_frame_slots": NFRAMES, "points": M, "observations": int(len(mp["obs_frame"]))},
            "search_level": LEVEL, "not_measured": ["hardware counters", "occupancy"]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"_meta": meta, "local_ba_device": rows}, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(meta, rows))


def markdown(meta, rows):
    g = lambda r, k: "%.3f (%.3f-%.3f)" % (r[k]["median_ms"], r[k]["p10_ms"], r[k]["p90_ms"])  # noqa: E731
    cols = ("device_route_one_wait", "device_route_stream_ms_per_call", "window_stream_ms_per_call", "local_ba_stream_ms_per_call", "host_route")
    out = ["# Local BA on the tables in device memory: window -> load -> optimise for batches of windows (tools/local_ba_device_bench.py)", "",
           "Commit: %s.  MI355X, one process, tables resident in device memory.  Map: %d key-frame slots, %d points, %d observations."
           % (meta["commit"], meta["map"]["key_frame_slots"], meta["map"]["points"], meta["map"]["observations"]),
           "A job = one current key frame, search_level %d, %d Levenberg-Marquardt iterations.  Device route: "
           "se2gpu_local_window_batch_device -> se2gpu_local_ba_batch_device, one wait.  Host route: the window call and a wait, the "
           "lists and the tables downloaded, flattened on the host (numpy), se2gpu_ba_load_local_graph + se2gpu_ba_initialize per "
           "window, one se2gpu_ba_optimize_batch under SE2GPU_BA_RESIDENT=1." % (meta["search_level"], rows[0]["iterations"]),
           "Milliseconds per batch, median (10th-90th percentile) over 7 windows of at least 0.3 s after two warm-up calls; "
           "\"on the stream\" = device events around 50 calls queued back to back, per call.", "",
           "| jobs | local / ref / free key frames, points, edges (mean) | device route, one wait | device route, on the stream | "
           "window, on the stream | local BA (gather + solve + finish), on the stream | host route |",
           "|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %.1f / %.1f / %.1f, %.0f, %.0f | " % (r["jobs"], r["local_kfs_mean"], r["ref_kfs_mean"], r["free_kfs_mean"],
                                                                 r["points_mean"], r["edges_mean"]) + " | ".join(g(r, k) for k in cols) + " |")
    out += ["", "Not measured: " + ", ".join(meta["not_measured"]) + ".", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
