#!/usr/bin/env python3
"""Feature constraints on tables in device memory: se2gpu_covis_pairs_device -> se2gpu_feat_edge_batch_device with one wait,
against the route a caller had before that call existed - pairs, wait, download of d_pair_out / d_common and of the table rows the
gather reads, the gather in numpy, se2gpu_feat_edge_batch - for 1 / 16 / 256 pairs of about 100 points.

    python tools/feat_edge_device_bench.py [--out profiles/feat_edge_device_bench.json]

Inputs: tests/feat_edge_device_cases.Tables over tests/feat_edge_cases.make_pair with 90 .. 110 points per pair (drawn per
pair, seed 7), covisibility mode, the reference's 15 iterations and minimum of 10 points.  Both routes start from the same
device tables and the same covisibility bit matrix and end with the constraints known to the host (the device route: after its
wait; its outputs stay in device memory).  Every shape is warmed first; the two routes alternate, window by window, in one
process; windows of at least 0.3 s; per route the median per-call time over the windows with the 10th and 90th percentile.
Reported besides: the baseline without its numpy gather (the gather timed alone), and the stream time of the new call alone
from device events.  The tables are built once for the largest batch; the baseline downloads only the rows its batch names
(the first 2 n frames, the batch's points and their observation entries - a prefix of every table), the smallest copy it can do."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feat_edge_device_cases as dc  # noqa: E402
from se2lam_amd import capi, covis, feat_edge as fe  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NPAIRS = [1, 16, 256]
LIST_CAP = ROW_CAP = 128
FTR_CAP = 128


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "p10_ms": ms[int(0.1 * (len(ms) - 1))], "p90_ms": ms[int(round(0.9 * (len(ms) - 1)))],
            "windows": len(ms)}


def window(fn, min_window):
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_window:
            return 1e3 * dt / n


def alternating(fns, min_window=0.3, windows=7):
    for f in fns:
        f(); f()
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            out[i].append(window(f, min_window))
    return [summary(o) for o in out]


def numpy_gather(pair_out, common, Twc, pos, obs_view, obs_info, pair_a, pair_b, row_cap):
    """the covisibility gather of tests/feat_edge_gather_model.py for in-range slots, vectorised: the arrays of
    se2gpu_feat_edge_batch"""
    n, list_cap = common.shape[:2]
    take = np.minimum(np.minimum(pair_out[:, 0], list_cap), row_cap)
    live = np.arange(list_cap)[None, :] < take[:, None]
    pt, ea, eb = common[..., 0], common[..., 1], common[..., 2]
    ok = live & (pt >= 0) & (pt < len(pos)) & (ea >= 0) & (ea < len(obs_view)) & (eb >= 0) & (eb < len(obs_view))
    mp_ptr = np.zeros(n + 1, np.int32)
    mp_ptr[1:] = np.cumsum(ok.sum(1))
    pt, ea, eb = pt[ok], ea[ok], eb[ok]
    T = Twc.astype(np.float64).reshape(-1, 3, 4)
    kf12 = lambda s: np.concatenate([T[s, :, :3].reshape(-1, 9), T[s, :, 3]], 1)   # noqa: E731
    kf = np.ascontiguousarray(np.stack([kf12(pair_a), kf12(pair_b)], 1))
    mp = np.ascontiguousarray(pos[pt], np.float64)
    z = np.ascontiguousarray(np.concatenate([obs_view[ea], obs_view[eb]], 1), np.float64)
    info = np.ascontiguousarray(np.concatenate([obs_info[ea], obs_info[eb]], 1), np.float64)
    return kf, mp_ptr, mp, z, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    lib, p = capi.lib(), capi.dev_ptr
    rng = np.random.default_rng(7)
    tab = dc.Tables([(int(rng.integers(90, 111)), 500 + i) for i in range(max(NPAIRS))])
    # the observation CSR of these tables: point g lists (frame 2w, feature j), (frame 2w + 1, feature j) - entries 2g, 2g + 1
    mp_ptr = (2 * np.arange(tab.m + 1)).astype(np.int32)
    obs_frame, obs_ftr = np.full(tab.nobs, -1, np.int32), np.zeros(tab.nobs, np.int32)
    for w in range(len(tab.N)):
        g = tab.off[w] + np.arange(tab.N[w])
        for k in range(2):
            obs_frame[2 * g + k], obs_ftr[2 * g + k] = 2 * w + k, np.arange(tab.N[w])
    matcher = ORBmatcher()
    cv = covis.build_device(matcher, np.full(tab.nframes, FTR_CAP, np.int32), FTR_CAP, mp_ptr, obs_frame, obs_ftr)
    d_Twc, d_pos, d_view, d_info = (capi.upload(x) for x in (tab.Twc, tab.pos, tab.obs_view, tab.obs_info))
    rows = []
    for n in NPAIRS:
        pair_a, pair_b = (2 * np.arange(n)).astype(np.int32), (2 * np.arange(n) + 1).astype(np.int32)
        npts = int(tab.off[n])      # the batch's worlds are the first n: a prefix of every table
        d_a, d_b = capi.upload(pair_a), capi.upload(pair_b)
        d_out, d_ratio = capi.upload(np.zeros((n, 4), np.int32)), capi.upload(np.zeros((n, 2), np.float32))
        d_common = capi.upload(np.zeros((n, LIST_CAP, 3), np.int32))
        buf = fe.FeatEdgeDeviceBuffers(n, ROW_CAP, poison=False)
        timer = capi.Timer()

        def pairs():
            capi.check(lib.se2gpu_covis_pairs_device(matcher._h, p(cv.bits), cv.nframes, cv.m, p(d_a), p(d_b), n, 0.3, 0.1, p(d_out),
                                                     p(d_ratio), p(d_common), LIST_CAP, p(cv.counts), cv.cap, p(cv.mp_ptr),
                                                     p(cv.obs_frame), p(cv.obs_ftr), cv.nobs))

        def device_call():
            capi.check(fe.feat_edge_batch_device(matcher, buf, fe.COVIS, d_a, d_b, tab.nframes, d_Twc, d_pos, tab.m,
                                                 covis=(d_out, d_common, LIST_CAP, d_view, d_info, tab.nobs)))

        def device_route():
            pairs()
            device_call()
            matcher.sync()

        def download():
            pairs()
            matcher.sync()
            # the rows this batch names and no more: its 2n frames, its points [0, off[n]) and their 2 off[n] observation entries
            return (d_out.to_numpy(np.int32, (n, 4)), d_common.to_numpy(np.int32, (n, LIST_CAP, 3)), d_Twc.to_numpy(np.float32, (2 * n, 12)),
                    d_pos.to_numpy(np.float32, (npts, 3)), d_view.to_numpy(np.float32, (2 * npts, 3)),
                    d_info.to_numpy(np.float32, (2 * npts, 9)))

        def baseline():
            flat = numpy_gather(*download(), pair_a, pair_b, ROW_CAP)
            rc, o = fe.feat_edge_raw(n, fe.COVIS, fe.COVIS_ITERS, fe.COVIS_MIN_POINTS, *flat)
            capi.check(rc)
            return o

        tables = download()
        flat0 = numpy_gather(*tables, pair_a, pair_b, ROW_CAP)

        def baseline_without_gather():
            download()
            capi.check(fe.feat_edge_raw(n, fe.COVIS, fe.COVIS_ITERS, fe.COVIS_MIN_POINTS, *flat0)[0])

        def gather_alone():
            numpy_gather(*tables, pair_a, pair_b, ROW_CAP)

        # both routes give a constraint for every pair, and the same one
        o = baseline()
        device_route()
        dev = buf.read()
        assert (o["info4"][:, 0] == 0).all() and all(d["status"] == 0 for d in dev), "every pair of the bench must produce a constraint"
        assert all(d["n_points"] == o["info4"][q, 1] for q, d in enumerate(dev))
        worst = max(np.abs(d["kf12"] - o["kf"][q]).max() for q, d in enumerate(dev))
        tb, td, tbg, tg = alternating([baseline, device_route, baseline_without_gather, gather_alone])
        ev = []
        for _ in range(60):
            pairs()
            timer.start(matcher.stream())
            device_call()
            timer.stop(matcher.stream())
            matcher.sync()
            ev.append(timer.elapsed_ms())
        ev = summary(ev[10:])
        row = {"pairs": n, "points": int(flat0[1][n]), "baseline": tb, "device_route": td, "baseline_without_gather": tbg, "numpy_gather": tg,
               "device_call_stream_ms": ev, "ws_bytes": buf.ws_bytes, "baseline_download_bytes": int(sum(t.nbytes for t in tables)), "poses_off_baseline": float(worst)}
        rows.append(row)
        print("%4d pairs (%5d points): baseline %.3f ms [%.3f, %.3f] (without the numpy gather %.3f, gather alone %.3f), device route "
              "%.3f ms [%.3f, %.3f], new call on the stream %.3f ms [%.3f, %.3f]"
              % (n, row["points"], tb["median_ms"], tb["p10_ms"], tb["p90_ms"], tbg["median_ms"], tg["median_ms"], td["median_ms"],
                 td["p10_ms"], td["p90_ms"], ev["median_ms"], ev["p10_ms"], ev["p90_ms"]), flush=True)
    res = {"mode": "covis", "iters": fe.COVIS_ITERS, "list_cap": LIST_CAP, "row_cap": ROW_CAP, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
