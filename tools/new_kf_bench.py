#!/usr/bin/env python3
"""A new key frame's observations for batches of key frames: se2gpu_kf_correspd_batch_device and
se2gpu_mappoint_parallax_batch_device with the data resident in device memory against the host functions of
include/se2lam_amd/FindCorrespd.h on ONE host thread over the same data (tools/new_kf_host.cpp, g++ -O2 -ffp-contract=off).

    python tools/new_kf_bench.py [--out profiles/new_kf.json]

Inputs (seed 7), per job three frames of 1,000 features (cap 1024): an old key frame (idkf 0, 0.3 to the left), the previous
one (idkf 3) and the new one (idkf 4, 0.15 to the right, turned by up to 1 degree); world points 2-6 deep, projected exactly
plus 0.2 px of noise.  700 features of the previous key frame are matched; 280 of them carry an observation (pass 1) that
the old key frame sees too, so their parallax update runs on three observations and promotes most of them; 420 are new
points (pass 3); 150 further features of the new key frame are matched to map points whose main observation is in the old
key frame (pass 2), a sixth of them with a normal 40 degrees off, so that the test refuses them.  1, 16 and 256 jobs.
Device: after two warm-up calls, windows of at least 0.3 s of call + se2gpu_matcher_sync (host clock) and device events
around 50 calls queued back to back; medians over 7 windows with the 10th / 90th percentile.  The observation call consumes
the hasObservation table, so every timed call starts from a fresh one: the host-clock windows upload it before each call
(timed alone as reset_and_sync), the 50 queued calls each work on a copy of their own that was uploaded before the events, and
the kinds the last of them counted must equal those of the first call.  The chain is passes = 1,
parallax, passes = 6: once queued on one stream with one wait, once with a wait and a download of kind / src / status after
every step and an upload of the match_idx_mp rows before the last one - the trip a caller makes who runs the steps in
between on the host.  The device's positions are compared with the host's before anything is timed.  No figure is gated."""
import argparse
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

from se2lam_amd import capi, newkf  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

CAP, NFEAT, FX, CX, CY, LOWER, UPPER = 1024, 1000, 230.0, 320.0, 240.0, 0.3, 100.0
N_MATCHED, N_TRACKED, N_MP = 700, 280, 150


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


def scene(B, rng):
    K = np.array([[FX, 0, CX], [0, FX, CY], [0, 0, 1.0]])
    nf = 3 * B
    kps = np.zeros(nf * CAP, capi.KP_DTYPE)
    kps["octave"] = 2
    Tcw, Twc, P = (np.zeros((nf, 12), np.float32) for _ in range(3))
    idkf = np.tile(np.array([0, 3, 4], np.int32), B)
    counts = np.full(nf, NFEAT, np.int32)
    observed = np.zeros(nf * CAP, np.uint8)
    view_pos = np.zeros((nf * CAP, 3), np.float32)
    matched12 = np.full((B, CAP), -1, np.int32)
    local_pos = np.zeros((B, CAP, 3), np.float32)
    midx = np.full((B, CAP), -1, np.int32)
    Tcr, Trc = np.zeros((B, 12), np.float32), np.zeros((B, 12), np.float32)
    mp = dict(main_frame=[], main_ftr=[], main_octave=[], normal=[], dist=[])
    lists = []
    for b in range(B):
        T64 = []
        for s, cx in enumerate((-0.3, 0.0, 0.15)):
            a = np.deg2rad(rng.uniform(-1, 1)) if s else 0.0
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, -R @ [cx, 0.01 * rng.standard_normal(), 0.0]
            T = T.astype(np.float32).astype(np.float64)
            f = 3 * b + s
            Tcw[f], Twc[f], P[f] = T[:3].ravel(), np.linalg.inv(T)[:3].ravel(), (K @ T[:3]).ravel()
            T64.append(T)
        Tn = T64[2] @ np.linalg.inv(T64[1])
        Tcr[b] = Tn[:3].ravel()
        Trc[b] = np.linalg.inv(np.vstack([Tcr[b].reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].ravel()
        X = np.stack([rng.uniform(-1.2, 1.2, NFEAT), rng.uniform(-0.8, 0.8, NFEAT), rng.uniform(2, 6, NFEAT), np.ones(NFEAT)], 1)
        perm = rng.permutation(NFEAT)
        for s in range(3):
            pc = (T64[s] @ X.T).T[:, :3]
            uv = (K @ (pc / pc[:, 2:]).T).T[:, :2] + 0.2 * rng.standard_normal((NFEAT, 2))
            idx = perm if s == 2 else np.arange(NFEAT)      # feature i of old and prev is point i; of new, point i is feature perm[i]
            o = (3 * b + s) * CAP + idx
            kps["x"][o], kps["y"][o] = uv[:, 0], uv[:, 1]
            if s == 1:
                view_pos[o[:N_TRACKED]] = pc[:N_TRACKED]
                local_pos[b, :NFEAT] = pc
        matched12[b, :N_MATCHED] = perm[:N_MATCHED]
        observed[(3 * b + 1) * CAP + np.arange(N_TRACKED)] = 1
        observed[(3 * b) * CAP + np.arange(N_TRACKED)] = 1
        for i in range(N_TRACKED):
            lists.append([(3 * b, i), (3 * b + 1, i), (3 * b + 2, int(perm[i]))])
        pcn = (T64[2] @ X.T).T[:, :3]
        for n, i in enumerate(range(N_MATCHED, N_MATCHED + N_MP)):   # points the matching did not pair: seen by old and new
            q = len(mp["main_frame"])
            d = np.linalg.norm(pcn[i])
            nv = pcn[i] / d
            if n % 6 == 5:
                a = np.deg2rad(40)
                nv = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ nv
            mp["main_frame"].append(3 * b); mp["main_ftr"].append(i); mp["main_octave"].append(2)
            mp["normal"].append(nv); mp["dist"].append([0.6 * d, 1.6 * d])
            midx[b, perm[i]] = q
    mp = dict(main_frame=np.array(mp["main_frame"], np.int32), main_ftr=np.array(mp["main_ftr"], np.int32),
              main_octave=np.array(mp["main_octave"], np.int32), normal=np.array(mp["normal"], np.float32),
              dist=np.array(mp["dist"], np.float32))
    ptr = (3 * np.arange(len(lists) + 1)).astype(np.int32)
    flat = np.array(lists, np.int32).reshape(-1, 2)
    return dict(kps=kps, counts=counts, Tcw=Tcw, Twc=Twc, P=P, idkf=idkf, observed=observed, view_pos=view_pos,
                job_prev=(3 * np.arange(B) + 1).astype(np.int32), job_new=(3 * np.arange(B) + 2).astype(np.int32), Tcr=Tcr, Trc=Trc,
                matched12=matched12, local_pos=local_pos, midx=midx, mp=mp, ptr=ptr, obs_frame=flat[:, 0].copy(),
                obs_ftr=flat[:, 1].copy(), new_frame=np.repeat(3 * np.arange(B) + 2, N_TRACKED).astype(np.int32))


class Resident:
    """everything of one scene in device memory, and the two calls on it without a transfer"""

    def __init__(self, s, mt):
        up = capi.upload
        self.s, self.mt, self.B = s, mt, len(s["job_prev"])
        self.poses = newkf.DevicePoses(s["kps"], s["counts"], CAP, s["Tcw"], s["Twc"], s["P"], s["idkf"], s["observed"], s["view_pos"])
        n, m, nobs = self.B * CAP, len(s["ptr"]) - 1, len(s["obs_frame"])
        self.n, self.m, self.nobs = n, m, nobs
        self.jobs = [up(s[k], dt) for k, dt in (("job_prev", np.int32), ("job_new", np.int32), ("Tcr", np.float32), ("Trc", np.float32),
                                                ("matched12", np.int32), ("local_pos", np.float32), ("midx", np.int32))]
        self.tab = [up(s["mp"][k], dt) for k, dt in (("main_frame", np.int32), ("main_ftr", np.int32), ("main_octave", np.int32),
                                                     ("normal", np.float32), ("dist", np.float32))]
        self.out = [up(np.zeros(n, np.int32), np.int32), up(np.zeros(n, np.uint8), np.uint8), up(np.zeros(n, np.int32), np.int32),
                    up(np.full((n, 3), -7.0), np.float32), up(np.zeros((n, 9)), np.float32), up(np.zeros((n, 3)), np.float32),
                    up(np.zeros((n, 9)), np.float32), up(np.zeros(5 * self.B, np.int32), np.int32)]
        self.lists = [up(s[k], np.int32) for k in ("ptr", "obs_frame", "obs_ftr", "new_frame")]
        self.good = up(np.zeros(m, np.uint8), np.uint8)
        self.tables = []
        self.pout = [up(np.zeros(m, np.int32), np.int32), up(np.zeros(m, np.int32), np.int32), up(np.zeros((m, 3)), np.float32),
                     up(np.zeros((nobs, 3)), np.float32), up(np.zeros((nobs, 9)), np.float32)]

    def reset(self):
        """the hasObservation table as it was before the first call (a blocking upload; timed on its own as reset_and_sync)"""
        capi.check(capi.lib().se2gpu_memcpy_h2d(self.poses.kf_observed.ptr, capi.vp(self.s["observed"]), self.s["observed"].nbytes))

    def fresh_tables(self, k):
        """k further copies of the hasObservation table as it was before the first call (blocking uploads)"""
        while len(self.tables) < k:
            self.tables.append(capi.DeviceArray(self.s["observed"].nbytes))
        for t in self.tables[:k]:
            capi.check(capi.lib().se2gpu_memcpy_h2d(t.ptr, capi.vp(self.s["observed"]), self.s["observed"].nbytes))
        return self.tables[:k]

    def correspd(self, passes, table=None):
        """the observation call on the resident table, or on `table` (a copy of it: the call consumes the flags)"""
        p = self.poses
        capi.check(capi.lib().se2gpu_kf_correspd_batch_device(
            self.mt._h, p.kps_un.ptr, p.counts.ptr, CAP, p.nframes, p.Tcw.ptr, p.Twc.ptr, p.P.ptr,
            (table or p.kf_observed).ptr, p.view_pos.ptr,
            *[x.ptr for x in self.jobs], self.B, *[x.ptr for x in self.tab], len(self.s["mp"]["main_frame"]), FX, LOWER, UPPER, passes,
            *[x.ptr for x in self.out]))

    def parallax(self):
        p = self.poses
        capi.check(capi.lib().se2gpu_mappoint_parallax_batch_device(
            self.mt._h, p.kps_un.ptr, p.counts.ptr, CAP, p.nframes, p.Tcw.ptr, p.Twc.ptr, p.P.ptr, p.idkf.ptr, self.lists[0].ptr,
            self.lists[1].ptr, self.lists[2].ptr, self.m, self.nobs, self.good.ptr, self.lists[3].ptr, FX, LOWER, UPPER,
            p.kf_observed.ptr, *[x.ptr for x in self.pout]))


def stream_ms(mt, fn, before=None):
    """device events around 50 calls queued back to back, per call; fn(k) queues the k-th, before() runs outside the events"""
    ev, timer = [], capi.Timer()
    for _ in range(7):
        if before:
            before()
        timer.start(mt.stream())
        for k in range(50):
            fn(k)
        timer.stop(mt.stream())
        mt.sync()
        ev.append(timer.elapsed_ms() / 50)
    ev.sort()
    return {"median_ms": ev[3], "p10_ms": ev[1], "p90_ms": ev[5]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,16,256")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    tmp = tempfile.mkdtemp(prefix="new_kf_")
    exe = os.path.join(tmp, "new_kf_host")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "new_kf_host.cpp"), "-o", exe, "-L", libdir, "-lse2gpu", "-Wl,-rpath," + libdir])
    mt = ORBmatcher()
    rows = []
    for B in [int(x) for x in a.sizes.split(",")]:
        s = scene(B, np.random.default_rng(7))
        r = Resident(s, mt)
        r.correspd(7)
        mt.sync()
        n = B * CAP
        kind, src = r.out[1].to_numpy(np.uint8, (n,)), r.out[2].to_numpy(np.int32, (n,))
        view = r.out[3].to_numpy(np.float32, (n, 3))
        cnt = r.out[7].to_numpy(np.int32, (B, 5))
        r.reset()
        r.parallax()
        mt.sync()
        status = r.pout[0].to_numpy(np.int32, (r.m,))
        d = os.path.join(tmp, str(B))
        os.makedirs(d)
        for name, arr in (("head.i32", np.array([3 * B, CAP, B, r.m, r.nobs], np.int32)), ("par.f32", np.array([FX, LOWER, UPPER], np.float32)),
                          ("counts.i32", s["counts"]), ("idkf.i32", s["idkf"]), ("Tcw.f32", s["Tcw"]), ("Twc.f32", s["Twc"]), ("P.f32", s["P"]),
                          ("kps.bin", s["kps"]), ("view_pos.f32", s["view_pos"]), ("local_pos.f32", s["local_pos"]),
                          ("job_prev.i32", s["job_prev"]), ("job_new.i32", s["job_new"]), ("Tcr.f32", s["Tcr"]), ("Trc.f32", s["Trc"]),
                          ("kind.u8", kind), ("src.i32", src), ("match_idx_mp.i32", s["midx"]), ("main_frame.i32", s["mp"]["main_frame"]),
                          ("main_ftr.i32", s["mp"]["main_ftr"]), ("main_octave.i32", s["mp"]["main_octave"]), ("normal.f32", s["mp"]["normal"]),
                          ("dist.f32", s["mp"]["dist"]), ("ptr.i32", s["ptr"]), ("obs_frame.i32", s["obs_frame"]), ("obs_ftr.i32", s["obs_ftr"]),
                          ("new_frame.i32", s["new_frame"])):
            np.ascontiguousarray(arr).tofile(os.path.join(d, name))
        host = subprocess.run([exe, d], capture_output=True, text=True, check=True).stdout.split()
        hv = np.fromfile(os.path.join(d, "host_view.f32"), np.float32).reshape(n, 3)
        assert np.array_equal(hv[:, 0] != -7.0, kind > 0), "device and host disagree on which features become observations"
        w = kind > 0
        assert (np.linalg.norm(hv[w].astype(np.float64) - view[w], axis=1) / np.linalg.norm(view[w], axis=1)).max() < 1e-5
        assert np.array_equal(np.fromfile(os.path.join(d, "host_status.i32"), np.int32), status)

        def one(passes):
            def f():
                r.reset()
                r.correspd(passes)
                mt.sync()
            return f

        def prl():
            r.parallax()
            mt.sync()

        def chain_one_wait():
            r.reset()
            r.correspd(1)
            r.parallax()
            r.correspd(6)
            mt.sync()

        def chain_host_trip():
            r.reset()
            r.correspd(1)
            mt.sync()
            r.out[1].to_numpy(np.uint8, (n,)); r.out[2].to_numpy(np.int32, (n,))
            r.parallax()
            mt.sync()
            r.pout[0].to_numpy(np.int32, (r.m,))
            capi.check(capi.lib().se2gpu_memcpy_h2d(r.jobs[6].ptr, capi.vp(s["midx"]), s["midx"].nbytes))
            r.correspd(6)
            mt.sync()
            r.out[1].to_numpy(np.uint8, (n,)); r.out[2].to_numpy(np.int32, (n,))

        def reset_only():
            r.reset()
            mt.sync()
        row = {"jobs": B, "features": B * NFEAT, "kinds": cnt[:, 1:4].sum(0).tolist(), "tracked_points": int(r.m),
               "promoted": int((status == 1).sum()),
               "reset_and_sync": windows(reset_only),
               "correspd_passes7_reset_call_and_sync": windows(one(7)),
               # the call consumes the flags: each of the 50 queued calls gets a table of its own, uploaded before the events
               "correspd_stream_ms_per_call": stream_ms(mt, lambda k: r.correspd(7, r.tables[k]), lambda: r.fresh_tables(50)),
               "correspd_stream_last_call_kinds": r.out[7].to_numpy(np.int32, (B, 5))[:, 1:4].sum(0).tolist(),
               "parallax_call_and_sync": windows(prl), "parallax_stream_ms_per_call": stream_ms(mt, lambda k: r.parallax()),
               "chain_one_wait": windows(chain_one_wait), "chain_with_host_trips": windows(chain_host_trip),
               "host_correspd_one_thread": {"median_ms": float(host[2]), "p10_ms": float(host[3]), "p90_ms": float(host[4])},
               "host_parallax_one_thread": {"median_ms": float(host[7]), "p10_ms": float(host[8]), "p90_ms": float(host[9])}}
        assert row["correspd_stream_last_call_kinds"] == row["kinds"], "the calls timed on the stream did not do the full work"
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"new_kf": rows}, f, indent=1)


if __name__ == "__main__":
    main()
