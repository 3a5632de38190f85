#!/usr/bin/env python3
"""Randomised parity sweep on the GPU (not part of the test suite: it runs for as long as it is given).
   python tools/fuzz_gpu.py [seconds] [seed] [kinds, comma separated]
ORB: random image sizes / feature counts / level counts / score types, single frames and batches against the oracle.
BA : random SE(2) windows (sizes, fixed patterns, kidnapped starts) - LM histories against the oracle; SE3-expmap windows under a
     random odometry / prior layout (synth.odometry_topology3), alone and in resident batches.
Prints one line per case and exits non-zero at the first mismatch."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oracle import oracle  # noqa: E402  (checker only)
from se2lam_amd import synth  # noqa: E402
from se2lam_amd.optimizer import SlamOptimizer  # noqa: E402
from se2lam_amd.orb import ORBextractor  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
KINDS = [int(k) for k in sys.argv[3].split(',')] if len(sys.argv) > 3 else list(range(16))   # e.g. 0,4,5: the three BA models only; 11 = the one-workgroup-per-window batch path; 12 = feature constraints; 13 = map points' main key frame; 14 = a new key frame's observations; 15 = covisibility
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t_end = time.time() + budget
tex = synth.texture()
ncase = 0
from se2lam_amd import optimizer as op  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402
from se2lam_amd.track import Track  # noqa: E402

feat_cache = {}
track = Track()


def feats(t):
    if t not in feat_cache:
        feat_cache[t] = oracle.orb_extract(synth.frame(t))
    return feat_cache[t]


def ba3_layout(g):
    """g under a random odometry / prior layout (synth.odometry_topology3), or as it is when the window cannot hold the one drawn"""
    kind = str(rng.choice(("chain",) + synth.ODOMETRY_TOPOLOGIES3))
    if kind == "chain":
        return g, kind
    try:
        return synth.odometry_topology3(g, kind, seed=int(rng.integers(1, 10**6))), kind
    except ValueError:
        return g, "chain"


def fail(msg):
    print(msg + " MISMATCH")
    sys.exit(1)


while time.time() < t_end:
    ncase += 1
    kind = KINDS[ncase % len(KINDS)]
    if kind == 2:   # MatchByWindow on feature subsets / windows / ratios, chained vbPrevMatched
        a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        (k1, d1), (k2, d2) = feats(a), feats(b)
        n1, n2 = int(rng.integers(0, len(k1) + 1)), int(rng.integers(0, len(k2) + 1))
        s1, s2 = np.sort(rng.choice(len(k1), n1, replace=False)), np.sort(rng.choice(len(k2), n2, replace=False))
        k1, d1, k2, d2 = k1[s1], np.ascontiguousarray(d1[s1]), k2[s2], np.ascontiguousarray(d2[s2])
        win, lo = int(rng.choice([5, 12, 20, 45, 90])), int(rng.integers(0, 3))
        mn = int(rng.integers(0, 3)); mx = int(rng.integers(mn + 1, 9)); ratio = float(rng.choice([0.6, 0.75, 0.9, 1.0]))
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32)
        # (no capacity left to refuse on: a window with more than 128 candidates takes the exact spill scan)
        nm, m12 = ORBmatcher(ratio).MatchByWindow(k1, d1, k2, d2, prev, win, lo, mn, mx)
        m_ref, nm_ref, p_ref = oracle.match_window(k1, d1, k2, d2, None, win, lo, mn, mx, ratio)
        ok = nm == nm_ref and np.array_equal(m12, m_ref) and np.array_equal(prev, p_ref)
        print(f"match frames {a}->{b} n {n1}x{n2} win {win} levels {mn}..{mx} ratio {ratio}: {nm} matches {'ok' if ok else ''}")
        if not ok:
            fail("match")
        continue
    if kind == 3:   # findFundamentalMat masks
        n = int(rng.choice([0, 5, 7, 8, 12, 14, 15, 16, 40, 300, 1000, 3001]))
        # synth.two_view_matches: the generator of tests/test_ransac.py / test_track_independent.py, with pure-inlier and
        # noise-free draws (the loop stops after a handful of samples) and up to 70 % outliers (it runs all 1000)
        frac = float(rng.choice([0.0, rng.uniform(0, 0.7), 0.7]))
        p1, p2, _ = synth.two_view_matches(int(rng.integers(0, 10**6)), n, frac, float(rng.choice([0.0, 0.5])))
        mask, ni = track.findFundamentalMat(p1, p2)
        mask_ref, info_ref = oracle.fundamental_mask_info(p1, p2)
        ok = ni == info_ref["inliers"] and np.array_equal(mask, mask_ref) and (n < 8 or track.last_ransac() == info_ref)
        print(f"ransac n {n} outliers {frac:.2f}: {ni} inliers {'ok' if ok else ''}")
        if not ok:
            fail("ransac")
        continue
    if kind == 4:   # marginalising SE3-expmap window
        P = int(rng.integers(3, 40)); L = int(rng.integers(2 * P, 30 * P)); nref = int(rng.integers(0, min(4, P - 2) + 1))
        g, layout = ba3_layout(synth.ba3_graph(P, L, nref, seed=int(rng.integers(1, 10**6))))
        o = op.SlamOptimizer(); op.load_se3_graph(o, g); o.initializeOptimization(0)
        iters = int(rng.integers(1, 11))
        o.optimize(iters)
        st = oracle.ba3_optimize(g, iters)[3]
        s_ = o.stats
        ok = s_["trials_hist"] == st["trials_hist"] and np.allclose(s_["chi2_hist"], st["chi2_hist"], rtol=1e-5, atol=0)
        print(f"ba3  P {P} L {L} ref {nref} E {g.E} O {g.O} {layout} iters {iters}: trials {s_['trials_hist']} {'ok' if ok else ''}")
        if not ok:
            fail("ba3")
        continue
    if kind == 5:   # pose graph
        P = int(rng.integers(3, 120))
        g = synth.pose_graph(P, seed=int(rng.integers(1, 10**6)))
        o = op.SlamOptimizer(); op.load_pose_graph(o, g); o.initializeOptimization(0)
        iters = int(rng.integers(1, 11))
        o.optimize(iters)
        st = oracle.pg_optimize(g, iters)[2]
        s_ = o.stats
        ok = s_["trials_hist"] == st["trials_hist"] and np.allclose(s_["chi2_hist"], st["chi2_hist"], rtol=1e-5, atol=0)
        print(f"pg   P {P} edges {g.O} iters {iters}: trials {s_['trials_hist']} {'ok' if ok else ''}")
        if not ok:
            fail("pg")
        continue
    if kind == 6:   # MatchByProjection: map points back-projected from one frame's key points, seen from a moved key frame
        a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        (k0, d0), (k1, d1) = feats(a), feats(b)
        m = int(rng.choice([0, 1, 40, 700, 1500, 3000]))
        src = rng.integers(0, len(k0), m)
        depth = rng.uniform(800, 6000, m).astype(np.float32)
        Xc = np.stack([(k0["x"][src] - 320.0) / 400.0 * depth, (k0["y"][src] - 240.0) / 400.0 * depth, depth], 1).astype(np.float32)
        th = float(rng.uniform(-0.03, 0.03))
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float32)
        tt = rng.uniform(-30, 30, 3).astype(np.float32)
        Tcw = np.concatenate([R, tt[:, None]], 1).astype(np.float32)
        mp_pos = ((Xc - tt) @ R).astype(np.float32)
        mp_desc = np.ascontiguousarray(d0[src].copy())
        flip = rng.integers(0, 256, (m, 32)).astype(np.uint8) & ((rng.random((m, 32)) < 0.03).astype(np.uint8) * 255)
        mp_desc ^= flip.astype(np.uint8)
        args = (mp_pos, mp_desc, k0["octave"][src].astype(np.int32), (rng.random(m) < 0.1).astype(np.uint8), Tcw,
                (400.0, 400.0, 320.0, 240.0), k1, d1, (rng.random(len(k1)) < 0.2).astype(np.uint8))
        win, lo = int(rng.choice([8, 15, 25])), int(rng.integers(0, 4))
        nm, idx = ORBmatcher().MatchByProjection(*args, win, lo)
        idx_ref, nm_ref = oracle.match_projection(*args, win, lo, 0.6)
        ok = nm == nm_ref and np.array_equal(idx, idx_ref)
        print(f"proj frames {a}->{b} map points {m} win {win} level offset {lo}: {nm} matches {'ok' if ok else ''}")
        if not ok:
            fail("proj")
        continue
    if kind == 7:   # doTriangulate
        n = int(rng.choice([0, 1, 30, 127, 128, 129, 600, 1000, 20000]))
        scene = str(rng.choice(list(synth.TRIANGULATION_SCENES)))      # benign, low parallax, far, behind the camera, zero baseline, noisy
        k1, k2, match, has_obs, P1, P2, Ocam, _ = synth.triangulation_scene(scene, n, int(rng.integers(0, 10**6)))
        match[rng.random(n) < 0.1] = -1
        has_obs = [(rng.random(n) < 0.15).astype(np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8), None][int(rng.integers(0, 4))]
        mind = int(rng.integers(1, 5))
        ref = oracle.triangulate(k1, k2, match, has_obs, P1, P2, Ocam, 500.0, 8000.0, mind)
        got = track.doTriangulate(k1, k2, match, has_obs, P1, P2, Ocam, 500.0, 8000.0, mind)
        ok = np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and got[3:] == ref[3:]
        print(f"tri  {scene} n {n} minDegree {mind}: {got[3]} good {'ok' if ok else ''}")
        if not ok:
            fail("tri")
        continue
    if kind == 8:   # Sparsifier::DoMarginalizeSE3XYZ, a batch of key-frame pairs
        from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
        spec = [(int(rng.integers(1, 250)), int(rng.integers(0, 10**6)), float(rng.uniform(80, 900))) for _ in range(int(rng.integers(1, 9)))]
        # each pair with its measurements in one of synth.KF_PAIR_ORDERS: the answer depends on the order (H11 is summed in it)
        pairs = [synth.kf_pair_reorder(synth.kf_pair(*sp), str(rng.choice(synth.KF_PAIR_ORDERS)), int(rng.integers(0, 10**6))) for sp in spec]
        got = DoMarginalizeSE3XYZ_batch(pairs)
        ok = True
        for sp, (kf, mp, m_kf, m_mp, m_info), (z, info) in zip(spec, pairs, got):
            zr, ir, _ = oracle.sparsify(kf, mp, m_kf, m_mp, m_info)
            good = np.allclose(z, zr, atol=1e-12) and np.abs(info - ir).max() <= 1e-5 * np.abs(ir).max()
            if not good:
                w = np.linalg.eigvalsh(0.5 * (ir + ir.T))
                print(f"spars pair {sp}: rel diff {np.abs(info - ir).max() / np.abs(ir).max():.3e}, z diff {np.abs(z - zr).max():.3e}, "
                      f"eig(info_ref) {w.min():.3e} .. {w.max():.3e}")
            ok = ok and good
        print(f"spars {len(pairs)} pairs: {'ok' if ok else ''}")
        if not ok:
            fail("spars")
        continue
    if kind == 9:   # Localizer::DoLocalBA (pose-only BA with the plane-motion prior)
        from se2lam_amd.localizer import Localizer
        TBC = np.eye(4); TBC[:3, :3] = synth.RBC; TBC[:3, 3] = synth.TBC
        n = int(rng.choice([0, 1, 3, 6, 40, 63, 64, 65, 255, 256, 257, 400, 1023, 1500]))
        # synth.pose_ba_case: headings next to +-pi, weights over 1 .. 1.2^-14 with exact zeros, a few points behind the camera
        kw = dict(outliers=float(rng.uniform(0, 0.3)), yaw=[None, np.pi - 5e-4, -np.pi + 5e-4][int(rng.integers(0, 3))],
                  weights=str(rng.choice(["levels", "wide"])), behind=int(rng.choice([0, 0, 3])))
        _, Tcw0, Xw, uv, w, pose = synth.pose_ba_case(int(rng.integers(0, 10**6)), n, **kw)
        delta = float(np.sqrt(5.991))
        loc = Localizer()
        T = loc.DoLocalBA(Tcw0, TBC, Xw, uv, w, 400.0, 320.0, 240.0, delta, 30)
        st = loc.stats
        meas, info = oracle.plane_motion_prior(Tcw0, TBC)
        To, so = oracle.pose_only_ba(Tcw0, meas, info, Xw, uv, w, 400.0, 320.0, 240.0, delta, 30)
        # identical trial counts and costs while the steps still change the cost (tests/test_pose_ba.py::_same_run)
        h = np.asarray(so["chi2_hist"]); prev = np.concatenate([[so["chi2_init"]], h[:-1]])
        flat = (prev - h) < 1e-9 * np.maximum(h, 1e-300)
        live = min(int(np.argmax(flat)) if flat.any() else len(h), st["iterations"])
        nn = min(st["iterations"], so["iterations"])
        noise = so["chi2_init"] < 1e-18      # only the prior edge, already at its minimum: the cost is rounding noise
        ok = (noise or np.isclose(st["chi2_init"], so["chi2_init"], rtol=1e-12) and list(st["trials_hist"][:live]) == list(so["trials_hist"][:live])
              and np.allclose(st["chi2_hist"][:nn], so["chi2_hist"][:nn], rtol=1e-5, atol=1e-12)) and (
              np.allclose(T[:3, :3], To[:3, :3], atol=1e-6) and np.allclose(T[:3, 3], To[:3, 3], rtol=1e-5, atol=1e-2))
        print(f"pose n {n}: {st['iterations']} iterations {'ok' if ok else ''}")
        if not ok:
            print(st, so)
            fail("pose")
        continue
    if kind == 10:   # SearchByBoW with a stand-in vocabulary (node = the first bits of the descriptor)
        a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        (k1, d1), (k2, d2) = feats(a), feats(b)
        nbits = int(rng.integers(1, 9))

        def fvec(desc, keep_p):
            node = (desc[:, 0].astype(np.int32) | (desc[:, 1].astype(np.int32) << 8)) & ((1 << nbits) - 1)
            order = np.argsort(node, kind="stable")
            nodes, counts = np.unique(node[order], return_counts=True)
            ptr = np.concatenate([[0], np.cumsum(counts)])
            keep = rng.random(len(nodes)) < keep_p
            segs = [order[ptr[i]:ptr[i + 1]] for i in range(len(nodes)) if keep[i]]
            return (nodes[keep].astype(np.int32), np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int32),
                    (np.concatenate(segs) if segs else np.zeros(0, np.int64)).astype(np.int32))
        fv1, fv2 = fvec(d1, rng.uniform(0.5, 1.0)), fvec(d2, rng.uniform(0.5, 1.0))
        h1 = (rng.random(len(k1)) < 0.7).astype(np.uint8); h2 = (rng.random(len(k2)) < 0.7).astype(np.uint8)
        ratio = float(rng.choice([0.6, 0.75, 0.9])); mp_only = bool(rng.integers(0, 2)); ori = bool(rng.integers(0, 2))
        nm, m12 = ORBmatcher(ratio).SearchByBoW(k1, d1, fv1, h1, k2, d2, fv2, h2, bIfMPOnly=mp_only, checkOri=ori)
        m_ref, nm_ref = oracle.search_by_bow(k1, d1, fv1, h1, k2, d2, fv2, h2, mp_only, ratio, ori)
        ok = nm == nm_ref and np.array_equal(m12, m_ref)
        print(f"bow  frames {a},{b} bits {nbits} mpOnly {mp_only} ori {ori} ratio {ratio}: {nm} matches {'ok' if ok else ''}")
        if not ok:
            fail("bow")
        continue
    if kind == 11:   # a batch of random windows through the one-workgroup-per-window kernels (csrc/ba_window.hip, ba_window3.hip)
        # SE(2) windows against the oracle; SE3-expmap windows (drawn half the time, up to 28 key frames) against the multi-launch path
        nb = int(rng.integers(1, 7))
        gs, its = [], int(rng.integers(1, 11))
        for _ in range(nb):
            if rng.random() < 0.5:
                P = int(rng.integers(3, 29)); nref = int(rng.integers(0, min(4, P - 2) + 1))
                gs.append(ba3_layout(synth.ba3_graph(P, int(rng.integers(2 * P, 30 * P)), nref, seed=int(rng.integers(1, 10**6))))[0])
                continue
            P = int(rng.integers(2, 61))
            L = int(rng.integers(max(8, P), 30 * P))
            g = synth.ba_graph(P, L, obs_per_lm=float(rng.uniform(2.5, 12.0)), seed=int(rng.integers(1, 10**6)))
            if rng.random() < 0.4:
                k = int(rng.integers(1, P))
                g.poses[k, :2] += rng.normal(0, 400, 2)
            gs.append(g)
        def opt_of(g):
            o = SlamOptimizer()
            if isinstance(g, synth.BA3Graph):
                op.load_se3_graph(o, g)
            else:
                o.load(g)
            o.initializeOptimization(0)
            return o
        os.environ["SE2GPU_BA_RESIDENT"] = "1"
        opts = [opt_of(g) for g in gs]
        op.optimize_batch(opts, its)
        os.environ.pop("SE2GPU_BA_RESIDENT")
        from se2lam_amd import capi as _capi
        path = int(_capi.lib().se2gpu_ba_last_batch_path())
        for g, o in zip(gs, opts):
            if isinstance(g, synth.BA3Graph):
                os.environ["SE2GPU_BA_RESIDENT"] = "0"
                m = opt_of(g)
                m.optimize(its)
                os.environ.pop("SE2GPU_BA_RESIDENT")
                st, n = m.stats, m.stats["iterations"]
                ok = o.stats["iterations"] == n and o.stats["trials_hist"][:n] == st["trials_hist"][:n] and \
                    np.allclose(o.stats["chi2_hist"][:n], st["chi2_hist"][:n], rtol=1e-9) and \
                    np.allclose(o.estimates()[0], m.estimates()[0], rtol=1e-9, atol=1e-9)
                print(f"baw3 path {path} P {g.P} L {g.L} E {g.E} iters {its}: trials {o.stats['trials_hist'][:n]} {'ok' if ok else 'MISMATCH'}")
                if not ok or path != 2:
                    print(o.stats["chi2_hist"][:n], st["chi2_hist"][:n], st["trials_hist"][:n])
                    sys.exit(1)
                continue
            ref = oracle.ba_optimize(g, its)[2]
            n = ref["iterations"]
            got, want = np.array(o.stats["chi2_hist"][:o.stats["iterations"]]), np.array(ref["chi2_hist"][:n])
            # a rejected / accepted trial whose gain ratio is within rounding of zero may fall either way when the sums are unordered:
            # the histories are compared while the decisions agree, and they must agree wherever |rho| is not tiny
            same = o.stats["iterations"] == n and o.stats["trials_hist"][:n] == ref["trials_hist"][:n]
            ok = same and np.allclose(got, want, rtol=1e-5)
            if not same and np.abs(np.array(ref["rho_log"])).min() < 1e-6:
                ok = True
            print(f"baw  path {path} P {g.P} L {g.L} E {g.E} iters {its}: trials {o.stats['trials_hist'][:o.stats['iterations']]} {'ok' if ok else 'MISMATCH'}")
            if not ok or path != 2:
                print(got, want, ref["trials_hist"][:n])
                sys.exit(1)
        continue
    if kind == 12:   # GlobalMapper::CreateFeatEdge: random N, mode and perturbation; the comparison is tests/test_feat_edge_gpu.py's
        tests_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
        if tests_dir not in sys.path:
            sys.path.insert(0, tests_dir)
        import feat_edge_cases as fc
        import feat_edge_model as fm
        from se2lam_amd import feat_edge as fe
        mode = int(rng.integers(0, 2))
        lo = fe.COVIS_MIN_POINTS if mode == fe.COVIS else fe.MATCH_MIN_POINTS
        spec = [dict(N=int(rng.integers(lo, 200)), seed=int(rng.integers(0, 10**6)), kf_sigma=(float(rng.uniform(1, 40)), float(rng.uniform(5e-4, 1e-2))),
                     mp_sigma=float(rng.uniform(1, 80))) for _ in range(int(rng.integers(1, 9)))]
        for sp in spec:
            sp["n_outliers"] = int(rng.integers(0, sp["N"] // 6 + 1)) if mode == fe.MATCH else 0
        cases = [fc.make_pair(**sp) for sp in spec]
        got = fe.CreateFeatEdgeBatch([fc.as_tuple(c) for c in cases], mode)
        for sp, c, r in zip(spec, cases, got):
            m = fm.optimize(fm.Problem(c["kf"], c["mp"], c["z"], c["info"], mode), fe.COVIS_ITERS if mode == fe.COVIS else fe.MATCH_ITERS)
            if not fm.inputs_ok(m, mode):   # an edge at the rejection threshold, or fewer than 10 comparable iterations: not a case
                print(f"featedge mode {mode} {sp}: skipped (the model's conditions on the inputs do not hold)")
                continue
            try:
                fm.check_against_model(r, c, m, mode, oracle, f"featedge mode {mode} N {sp['N']} seed {sp['seed']}")
            except AssertionError:
                import traceback
                traceback.print_exc()
                fail(f"featedge mode {mode} {sp}")
        print(f"featedge mode {mode} {len(spec)} pairs: ok")
        continue
    if kind == 13:   # MapPoint::updateMainKFandDescriptor: random observation lists, planted duplicate descriptors, against the numpy model
        tests_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
        if tests_dir not in sys.path:
            sys.path.insert(0, tests_dir)
        import mappoint_main_model as mm
        from se2lam_amd import capi, mappoint as mpt
        nf, cap, nl = int(rng.integers(1, 200)), int(rng.integers(1, 33)), int(rng.integers(1, 9))
        n = nf * cap
        counts = rng.integers(0, cap + 3, nf).astype(np.int32)
        kps = np.zeros(n, capi.KP_DTYPE)
        kps["octave"] = rng.integers(-1, nl + 1, n)
        ndist = int(rng.choice([1, 2, 3, 8, 50, n]))     # few distinct descriptors: many rows share the least median
        desc = rng.integers(0, 256, (ndist, 32), dtype=np.uint8)[rng.integers(0, ndist, n)]
        desc ^= np.packbits(rng.random((n, 256)) < float(rng.choice([0.0, 0.0, 0.02, 0.2])), axis=1)
        view = (rng.standard_normal((n, 3)) * float(rng.uniform(0.1, 100))).astype(np.float32)
        null = (rng.random(nf) < float(rng.choice([0.0, 0.1, 0.9]))).astype(np.uint8)
        sf = (np.float32(rng.uniform(1.05, 1.5)) ** np.arange(nl)).astype(np.float32)
        m = int(rng.integers(1, 300))
        lens = np.where(rng.random(m) < 0.03, rng.integers(60, 400, m), np.minimum(rng.geometric(1 / 6.0, m) - 1, 70))
        lists = [(rng.integers(-1, nf + 1, L).astype(np.int32), rng.integers(-1, cap + 1, L).astype(np.int32)) for L in lens]
        prev = rng.integers(-1, nf, m).astype(np.int32) if rng.random() < 0.7 else None
        with_view = bool(rng.random() < 0.8)
        frames = mpt.DeviceFrames(kps, desc, counts, cap, null, view)
        batch = mpt.MainBatch(lists, prev)
        mt = ORBmatcher()
        batch.run(mt, frames, sf, with_view)
        got = batch.download(mt)
        ptr, fr, ft = mpt.csr(lists)
        want = mm.update_main_batch(kps, desc, counts, cap, nf, null, view if with_view else None, sf, nl, ptr, fr, ft, prev,
                                    mpt.sentinels(m))
        ok = all(np.array_equal(got[k], want[k]) for k in ("info", "main_desc", "main_frame", "main_octave")) and \
            np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32))
        print(f"mappoint main {nf} frames x {cap}, {m} points, {len(fr)} observations (longest {int(lens.max())}), {ndist} descriptors: "
              f"{int((want['info'][:, 0] >= 0).sum())} with a main {'ok' if ok else ''}")
        if not ok:
            fail("mappoint main")
        continue
    if kind == 14:   # updateParallax and findCorrespd: the scenes of tests/new_kf_cases.py under a random seed, against the FP64 model
        tests_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
        if tests_dir not in sys.path:
            sys.path.insert(0, tests_dir)
        import new_kf_cases as nc
        import new_kf_model as nk
        from se2lam_amd import newkf
        seed = int(rng.integers(1, 10**6))
        try:
            pc, cc = nc.ParallaxCases(seed), nc.CorrespdCases(seed, abandoned=bool(rng.random() < 0.5))
        except AssertionError as e:     # a scene in which some named case finds no draw with its margins
            print(f"new key frame seed {seed}: skipped ({e})")
            continue
        e_pos, e_mat = nc.restatement_errors(pc, [cc])
        bound = 4 * max(e_pos, e_mat)
        mt = ORBmatcher()
        fr = pc.sc.fr
        poses = newkf.DevicePoses(fr.kps, fr.counts, fr.cap, fr.Tcw, fr.Twc, fr.P, fr.idkf, pc.observed)
        got = newkf.promote_batch_device(mt, poses, pc.ptr, pc.obs_frame, pc.obs_ftr, pc.good, pc.new, nc.FX, nc.LOWER, nc.UPPER)
        want = pc.run(nk.L64)
        w = want["obs_view"][:, 0] != nk.SENT
        ok = np.array_equal(got["status"], want["status"]) and np.array_equal(got["place"], want["place"]) and \
            np.array_equal(poses.observed(), want["kf_observed"]) and \
            np.array_equal(got["obs_view"][:, 0] != np.float32(nk.SENT), w) and \
            nk.rel_err_pos(got["obs_view"][w], want["obs_view"][w]).max() <= bound and \
            nk.rel_err_mat(got["obs_info"][w], want["obs_info"][w]).max() <= bound
        passes = int(rng.integers(1, 8))
        fr = cc.sc.fr
        poses = newkf.DevicePoses(fr.kps, fr.counts, fr.cap, fr.Tcw, fr.Twc, fr.P, fr.idkf, cc.observed, cc.view_pos)
        got = newkf.observe_batch_device(mt, poses, cc.job_prev, cc.job_new, cc.Tcr, cc.Trc, cc.matched12, cc.local_pos,
                                         cc.match_idx_mp, cc.mp, nc.FX, nc.LOWER, nc.UPPER, passes)
        want = cc.run(nk.L64, passes)
        w = want["kind"] > 0
        ok = ok and all(np.array_equal(got[k], want[k]) for k in ("inv", "kind", "src", "counts")) and \
            np.array_equal(poses.observed(), want["kf_observed"]) and \
            (not w.any() or (nk.rel_err_pos(got["view"][w], want["view"][w]).max() <= bound and
                             nk.rel_err_mat(got["info"][w], want["info"][w]).max() <= bound))
        print(f"new key frame seed {seed}: {int((pc.run(nk.L64)['status'] == 1).sum())} promoted, passes {passes} kinds "
              f"{want['counts'][:, 1:4].sum(0).tolist()}, bound {bound:.2g} {'ok' if ok else ''}")
        if not ok:
            fail("new key frame")
        continue
    if kind == 15:   # Map::compareViewMPs in both overloads: random maps with planted irregularities, against the set model
        tests_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
        if tests_dir not in sys.path:
            sys.path.insert(0, tests_dir)
        import covis_cases as cvc
        import covis_model as cvm
        from se2lam_amd import covis
        seed, nf, m = int(rng.integers(1, 10**6)), int(rng.integers(1, 90)), int(rng.integers(0, 6000))
        t = cvc.random_map(seed, nf, m, irregular=bool(rng.random() < 0.8))
        model = cvm.Model(*cvc.tables(t))
        mt = ORBmatcher()
        cv = covis.build_device(mt, *cvc.tables(t))
        ok = np.array_equal(cv.read_bits(), model.bits()) and (m == 0 or np.array_equal(cv.read_size_obs(), model.size_obs()))
        pa, pb = cvc.pair_list(seed, nf, int(rng.integers(1, 60)))
        list_cap = [None, 0, int(rng.integers(1, 50)), m + 1][int(rng.integers(0, 4))]
        rf, rd = float(rng.choice([0.3, rng.random()])), float(rng.choice([0.1, rng.random()]))
        got, want = covis.pairs_device(mt, cv, pa, pb, rf, rd, list_cap), model.pairs(pa, pb, rf, rd, list_cap)
        ok = ok and np.array_equal(got["out"], want["out"]) and cvm.same_floats(got["ratio"], want["ratio"]) and \
            (list_cap is None or np.array_equal(got["common"], want["common"]))
        kf, rp, ri = cvc.job_list(seed + 1, nf, int(rng.integers(3, 40)), int(rng.integers(0, 100)))
        k, th = int(rng.integers(1, 8)), float(rng.choice([0.8, rng.random()]))
        gotj, wantj = covis.refset_device(mt, cv, kf, rp, ri, k, th), model.refset(kf, rp, ri, k, th)
        ok = ok and np.array_equal(gotj["out"], wantj["out"]) and cvm.same_floats(gotj["ratio"], wantj["ratio"])
        print(f"covisibility seed {seed}: {nf} key frames, {m} points, {len(pa)} pairs (list_cap {list_cap}), {len(kf)} jobs k {k} "
              f"{'ok' if ok else ''}")
        if not ok:
            fail("covisibility")
        continue
    if kind == 1:
        W, H = int(rng.integers(160, 900)), int(rng.integers(120, 700))
        nf = int(rng.choice([150, 500, 1000, 2000]))
        nl = int(rng.integers(1, 9))
        st = int(rng.integers(0, 2))
        B = int(rng.choice([1, 1, 3, 16, 21]))
        # the smallest level must keep a scan area (the library refuses otherwise, like the reference would crash)
        if min(W, H) / 1.2 ** (nl - 1) < 2 * 16 + 8:
            continue
        imgs = []
        for b in range(B):
            ox, oy = int(rng.integers(0, 1280 - W)), int(rng.integers(0, 960 - H))
            imgs.append(np.ascontiguousarray(tex[oy:oy + H, ox:ox + W]))
        try:
            ex = ORBextractor(nfeatures=nf, nlevels=nl, scoreType=st, max_rows=H, max_cols=W, max_batch=B)
        except Exception as e:   # geometry the library refuses: since round 5 only where the reference itself raises (a cell
            # window outside its level, cv::Mat::colRange) - checked against the compiled reference where it is present - or
            # where a level has more than 1024 cells
            msg = str(e)
            verdict = ""
            if "the reference raises" in msg:
                try:
                    from oracle import ref
                    if ref.available():
                        try:
                            ref.orb_extract(imgs[0], oracle.orb_params(nfeatures=nf, nlevels=nl, score_type=st), cap=4 * nf + 64)
                            print(f"orb  {W}x{H} nf {nf} levels {nl}: refused, but the compiled reference runs it MISMATCH")
                            sys.exit(1)
                        except ValueError:
                            verdict = " - and the compiled reference raises"
                except ImportError:
                    pass
            print(f"orb  {W}x{H} nf {nf} levels {nl}: refused ({msg[:90]}){verdict}")
            continue
        try:
            out = ex.extract_batch(np.stack(imgs)) if B > 1 else [ex(imgs[0])]
        except Exception as e:
            # (HARRIS_SCORE cells with more than 4096 corners are selected in bands of rows now: no capacity to refuse on)
            print(f"orb  {W}x{H} nf {nf} levels {nl} score {st} batch {B}: ERROR {str(e)[:100]}")
            sys.exit(1)
        p = oracle.orb_params(nfeatures=nf, nlevels=nl, score_type=st)
        for b in sorted({0, B - 1}):
            ko, do = oracle.orb_extract(imgs[b], p, cap=4 * nf + 64)
            ok = np.array_equal(out[b][0], ko) and np.array_equal(out[b][1], do)
            print(f"orb  {W}x{H} nf {nf} levels {nl} score {st} batch {B} frame {b}: {len(ko)} kp {'ok' if ok else 'MISMATCH'}")
            if not ok:
                sys.exit(1)
    else:
        big = rng.random() < 0.25    # loops long enough for the nested-dissection orders of the pose solve (several levels)
        P = int(rng.integers(70, 190)) if big else int(rng.integers(2, 70))
        L = int(rng.integers(max(8, P), (12 if big else 40) * P))
        g = synth.ba_graph(P, L, obs_per_lm=float(rng.uniform(2.5, 9.0)), seed=int(rng.integers(1, 10**6)))
        if rng.random() < 0.4:   # a start far from the optimum: rejected trials
            k = int(rng.integers(1, P))
            g.poses[k, :2] += rng.normal(0, 400, 2)
        iters = int(rng.integers(1, 12))
        o = SlamOptimizer()
        o.load(g)
        o.initializeOptimization(0)
        o.optimize(iters)
        ref = oracle.ba_optimize(g, iters)[2]
        got, want = np.array(o.stats["chi2_hist"][:o.stats["iterations"]]), np.array(ref["chi2_hist"][:ref["iterations"]])
        ok = (o.stats["iterations"] == ref["iterations"] and o.stats["trials_hist"][:ref["iterations"]] == ref["trials_hist"][:ref["iterations"]]
              and np.allclose(got, want, rtol=1e-5))
        print(f"ba   P {P} L {L} E {g.E} iters {iters}: trials {o.stats['trials_hist'][:o.stats['iterations']]} {'ok' if ok else 'MISMATCH'}")
        if not ok:
            print(got, want, ref["trials_hist"][:ref["iterations"]])
            sys.exit(1)
print(f"{ncase} cases, no mismatch")
