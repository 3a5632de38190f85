"""Bundle-adjustment graphs, handles and helpers that more than one test module uses (as tests/pg_cases.py does for the pose
graph): no tests, no fixtures.  A module that is also the script of its own child process imports this one first - it puts the
repository root on sys.path, which nothing has done in a bare `python tests/test_x.py`."""
import contextlib
import copy
import dataclasses
import os
import sys
import threading

import numpy as np

import scaled_parity as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- handles ----------------------------------------------------------------------------------------------------------------
def opt(g):
    """an initialised SE(2) handle of the window `g`"""
    from se2lam_amd.optimizer import SlamOptimizer
    o = SlamOptimizer()
    o.load(g)
    o.initializeOptimization(0)
    return o


def opt3(g):
    """an initialised SE3-expmap handle"""
    from se2lam_amd import optimizer as op
    o = op.SlamOptimizer()
    op.load_se3_graph(o, g)
    o.initializeOptimization(0)
    return o


def pg(g):
    """an initialised pose-graph handle"""
    from se2lam_amd import optimizer as op
    o = op.SlamOptimizer()
    op.load_pose_graph(o, g)
    o.initializeOptimization(0)
    return o


# ---- bounds -----------------------------------------------------------------------------------------------------------------
REL = 1e-5      # BASELINE.json north_star: BA cost and pose updates within 1e-5 relative


def pose_update_close(p_gpu, p_ref, p0, rel=REL):
    """pose UPDATES (estimate - initial) agree within `rel` relative (norm-wise per component)."""
    d_gpu, d_ref = p_gpu - p0, p_ref - p0
    for c in range(3):
        scale = np.abs(d_ref[:, c]).max() + 1e-12
        assert np.abs(d_gpu[:, c] - d_ref[:, c]).max() <= rel * scale, (c, np.abs(d_gpu[:, c] - d_ref[:, c]).max(), scale)


# ---- the environment --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def env(**kw):
    """environment variables for the body (None: unset), put back afterwards - for the switches the library reads per call
    (SE2GPU_BA_RESIDENT) or at every initialize (SE2GPU_BA_CHOL, SE2GPU_BA_PLAN)"""
    def put(k, v):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            put(k, v)
        yield
    finally:
        for k, v in old.items():
            put(k, v)


def multi_launch(g, iters, mode=0, make=opt):
    """one optimize() on the multi-launch path: stats, estimates and (SE3) the chi2() of every projection edge afterwards"""
    from se2lam_amd import optimizer as op
    with env(SE2GPU_BA_RESIDENT="0"):
        o = make(g)
        o.optimize(iters, mode)
        return o.stats, o.estimates(), (op.edgeChi2(o, g.E) if make is opt3 else None)


# ---- starts on which Levenberg-Marquardt rejects trials ---------------------------------------------------------------------
def kidnapped(synth, P, L, dxy, dth, nbad, seed):
    """A few key frames displaced by metres / tens of degrees (landmarks untouched, so no point comes near a camera
    plane): the Gauss-Newton-like first steps overshoot and Levenberg-Marquardt has to REJECT trials."""
    g = copy.copy(synth.ba_graph(P, L))   # the generator caches its graphs: never modify the shared instance
    rng = np.random.default_rng(seed)
    g.poses = g.poses.copy()
    idx = rng.choice(np.arange(1, g.P), nbad, replace=False)
    g.poses[idx, :2] += rng.normal(0, dxy, (nbad, 2))
    g.poses[idx, 2] += rng.normal(0, dth, nbad)
    # headings stay in [-pi, pi): the reference's Se2 normalises on construction (src/Config.cpp), and an out-of-range
    # theta would meet PreEdgeSE2's missing angle wrap (EdgeSE2XYZ.h:80) as a 2 pi cost jump at the first oplus
    g.poses[:, 2] = (g.poses[:, 2] + np.pi) % (2 * np.pi) - np.pi
    return g


# (P, L, dxy [mm], dtheta [rad], displaced key frames, seed) -> the trials per iteration of g2o's policy on that start.
# Chosen (tools-free search over seeds) so that EVERY accept / reject decision has a wide margin: |rho| >= 0.4 in all
# trials, where rho = 0 is the decision boundary - the last bits of the host libm cannot flip one - and no observed
# point is closer than 0.9 m to its camera plane at the start.
LM_REJECT_CASES = [
    ((8, 60, 2000.0, 0.8, 1, 4), [1, 1, 6, 5, 1, 3, 2, 3, 4, 3]),
    ((8, 60, 3000.0, 0.3, 4, 6), [1, 7, 1, 1, 1, 1, 1, 1, 1, 1]),
    ((21, 800, 3000.0, 0.3, 4, 13), [1, 1, 1, 1, 1, 8, 1, 1, 4, 1]),
    ((50, 5000, 3000.0, 0.3, 4, 12), [1, 7, 1, 1, 3, 2, 4, 3, 3, 3]),
    ((50, 5000, 3000.0, 0.3, 2, 23), [1, 1, 7, 1, 1, 3, 3, 2, 3, 4]),
]


def kidnapped3(synth, P, L, n_ref, dxy, dth, nbad, seed):
    """an SE3 window whose start has a few key frames moved by metres and tens of degrees in the plane: LM rejects trials"""
    g = copy.copy(synth.ba3_graph(P, L, n_ref))
    rng = np.random.default_rng(seed)
    g.poses = g.poses.copy()
    for a in rng.choice(np.arange(1, g.P - n_ref), nbad, replace=False):
        th = rng.normal(0, dth)
        M = np.eye(4)
        M[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        M[:2, 3] = rng.normal(0, dxy, 2)
        g.poses[a] = g.poses[a] @ M
    return g


REJECT = (21, 800, 0, 3000.0, 0.8, 2, 3)   # kidnapped3's arguments; the oracle: trials [1, 1, 6, 3, 1, 3, 2, 3, 1, 2]


# ---- SE(2) windows, each for a branch of the multi-launch kernels (csrc/ba.hip) or of the resident one (csrc/ba_window.hip) ---
def no_odometry(synth):
    """O = 0: the paths without a PreEdgeSE2 term.  Without those edges one fixed key frame leaves the scale of the window free,
    and Gauss-Newton (no damping) then factorises a singular system; a second fixed key frame takes that freedom away, so LM and
    GN are both well posed."""
    g = synth.ba_graph(30, 2000)
    fx = g.fixed.copy()
    fx[1] = 1
    return dataclasses.replace(g, fixed=fx, o_i=g.o_i[:0], o_j=g.o_j[:0], o_meas=g.o_meas[:0], o_info=g.o_info[:0])


def bare_pose(synth, pose=2):
    """key frame `pose` of ba_graph(30, 2000) keeps its two PreEdgeSE2 edges and loses every EdgeSE2XYZ: its wave of k_lambda0
    gathers nothing, its blocks have an edge and no pairs.  Key frame 2 is one whose edges can go while every landmark keeps two
    observations: a landmark with one has a singular block, which Gauss-Newton cannot invert."""
    g = synth.ba_graph(30, 2000)
    keep = g.e_kf != pose
    assert 0 < keep.sum() < g.E and not g.fixed[pose] and np.bincount(g.e_lm[keep], minlength=g.L).min() >= 2
    return dataclasses.replace(g, e_kf=g.e_kf[keep], e_lm=g.e_lm[keep], e_uv=g.e_uv[keep], e_info=g.e_info[keep])


DENSE_KFS, DENSE_LMS = (10, 11, 12, 13), 500


def dense_window(synth):
    """four neighbouring key frames of ba_graph(50, 5000), the first fixed, that ALL observe the same 500 landmarks: each of the
    three blocks between free key frames has 500 contributor pairs, more than 28 chunks of 16 (kGrpPerWG, kChunk), so its chunks
    are longer than the sixteen pairs a flat record holds and no block is empty; block (0, 1) has an edge, a fixed end and no
    pairs; one edge runs b -> a"""
    g = synth.ba_graph(50, 5000)
    kfs = list(DENSE_KFS)
    P = len(kfs)
    Rcb = synth.RBC.T
    tcb = -Rcb @ synth.TBC
    kf, lm = np.repeat(np.arange(P), g.L), np.tile(np.arange(g.L), P)
    u, v, z, _ = synth._project(g.poses_true[kfs], g.lms_true, kf, lm, Rcb, tcb, synth.FX, synth.CX, synth.CY)
    vis = ((z >= 300.0) & (z <= 12000.0) & (u >= 0) & (u < synth.IMG_W) & (v >= 0) & (v < synth.IMG_H)).reshape(P, -1)
    pick = np.nonzero(vis.all(axis=0))[0][:DENSE_LMS]
    assert pick.size == DENSE_LMS > 28 * 16
    rng = np.random.default_rng(77)
    e_lm = np.repeat(np.arange(DENSE_LMS), P).astype(np.int32)
    e_kf = np.tile(np.arange(P), DENSE_LMS).astype(np.int32)
    lms_t, poses_t = g.lms_true[pick], g.poses_true[kfs]
    u, v, _, _ = synth._project(poses_t, lms_t, e_kf, e_lm, Rcb, tcb, synth.FX, synth.CX, synth.CY)
    level = rng.integers(0, 8, e_kf.size)
    e_uv = np.stack([u, v], axis=1) + rng.normal(0.0, 1.0, (e_kf.size, 2)) * (1.2 ** level)[:, None]
    poses0, lms0 = g.poses[kfs].copy(), g.lms[pick].copy()
    fixed = np.array([1, 0, 0, 0], np.uint8)
    w = synth.BAGraph(poses=poses0, fixed=fixed, lms=lms0, e_kf=e_kf, e_lm=e_lm, e_uv=e_uv,
                      e_info=synth.edge_information(poses0, lms0, e_kf, e_lm, level, synth.RBC, synth.TBC, synth.FX),
                      o_i=np.zeros(0, np.int32), o_j=np.zeros(0, np.int32), o_meas=np.zeros((0, 3)), o_info=np.zeros((0, 9)),
                      poses_true=poses_t, lms_true=lms_t, e_level=level.astype(np.int32))
    return synth.with_odometry(w, [(0, 1), (2, 1), (2, 3)], seed=5)


def keep_edges(g, keep):
    """the graph with the edges `keep` and the landmarks that still have two of them (a landmark with one observation has a
    singular block)"""
    n = np.bincount(g.e_lm[keep], minlength=g.L)
    keep = keep & (n[g.e_lm] >= 2)
    lm_keep = np.nonzero(n >= 2)[0]
    remap = -np.ones(g.L, np.int64)
    remap[lm_keep] = np.arange(lm_keep.size)
    return dataclasses.replace(g, lms=g.lms[lm_keep].copy(), e_kf=g.e_kf[keep].copy(), e_lm=remap[g.e_lm[keep]].astype(np.int32),
                               e_uv=g.e_uv[keep].copy(), e_info=g.e_info[keep].copy(), lms_true=g.lms_true[lm_keep].copy(),
                               e_level=g.e_level[keep].copy())


def thin(synth):
    """ba_graph(30, 2000) keeping only the edges whose key frame lies within 2 of the landmark's first key frame: most blocks of
    the reduced system are empty (whole workgroups of k_reduce2 with nothing to do), three block columns in the solve"""
    g = synth.ba_graph(30, 2000)
    first = np.full(g.L, g.P, np.int64)
    np.minimum.at(first, g.e_lm, g.e_kf)
    return keep_edges(g, g.e_kf - first[g.e_lm] <= 2)


def thin4(synth):
    """a thin window with the dense window's four key frames: 0, 1, 12, 13 of `thin` (0 fixed), chained by three PreEdgeSE2
    edges: blocks (0, 2), (0, 3), (1, 3) are empty, (1, 2) has an edge and no pairs, (2, 3) has pairs"""
    g = thin(synth)
    kfs = np.array([0, 1, 12, 13])
    remap = -np.ones(g.P, np.int64)
    remap[kfs] = np.arange(4)
    w = keep_edges(g, np.isin(g.e_kf, kfs))
    w = dataclasses.replace(w, poses=g.poses[kfs].copy(), fixed=g.fixed[kfs].copy(), poses_true=g.poses_true[kfs].copy(),
                            e_kf=remap[w.e_kf].astype(np.int32))
    return synth.with_odometry(w, [(0, 1), (1, 2), (2, 3)], seed=3)


def merged_landmarks(synth, P=40, L=240, groups=12, per_group=3):
    """landmarks with 17 to 64 observations (the wave-per-landmark class of the resident kernel): the generator's landmarks are
    seen from a dozen neighbouring key frames at most, so `per_group` landmarks whose observers do not overlap are fused into one -
    its observations then disagree about where it is, which the robust least squares takes like any other outlier-ridden point"""
    g = copy.copy(synth.ba_graph(P, L))
    e_kf, e_lm = np.asarray(g.e_kf).copy(), np.asarray(g.e_lm).copy()
    seen = [set(e_kf[e_lm == l].tolist()) for l in range(g.L)]
    used, fused = set(), 0
    for a in range(g.L):
        if fused == groups:
            break
        if a in used:
            continue
        members, kfs = [a], set(seen[a])
        for b in range(a + 1, g.L):
            if b not in used and not (kfs & seen[b]):
                members.append(b)
                kfs |= seen[b]
                if len(members) == per_group:
                    break
        if len(members) == per_group:
            used.update(members)
            for b in members[1:]:
                e_lm[e_lm == b] = a
            fused += 1
    assert fused == groups
    keep = np.unique(e_lm)                       # the fused-away landmarks leave the graph
    renum = np.full(g.L, -1, np.int64)
    renum[keep] = np.arange(len(keep))
    e_lm = renum[e_lm]
    g.lms = np.asarray(g.lms)[keep].copy()
    if g.lms_true is not None:
        g.lms_true = np.asarray(g.lms_true)[keep].copy()
    order = np.argsort(e_lm, kind="stable")
    g.e_kf, g.e_lm = e_kf[order].astype(np.int32), e_lm[order].astype(np.int32)
    g.e_uv, g.e_info = np.asarray(g.e_uv)[order].copy(), np.asarray(g.e_info)[order].copy()
    return g


# ---- odometry graphs beyond the chain (synth.odometry_topology), SE(2) ------------------------------------------------------
def odometry_cases(synth, sizes):
    """(P, L, kind) of every odometry topology that a window of P key frames can hold (a hub of N edges needs N + 1 of them)"""
    return [(P, L, kind) for P, L in sizes for kind in synth.ODOMETRY_TOPOLOGIES
            if not (kind.startswith("hub") and int(kind[3:]) + 1 > P)]


def assert_topology(synth, g, kind):
    """the odometry of `g` has the shape synth.odometry_topology(.., kind) claims"""
    P = g.P
    oi, oj = np.asarray(g.o_i, np.int64), np.asarray(g.o_j, np.int64)
    und = sorted(zip(np.minimum(oi, oj).tolist(), np.maximum(oi, oj).tolist()))
    chain = [(k, k + 1) for k in range(P - 1)]
    cov = synth.covisible(g)
    far = [(i, j) for i, j in zip(oi, oj) if abs(i - j) >= 2 and not cov[i, j]]
    dup = len(set(und)) < len(und)
    loops = int((oi == oj).sum())
    if kind == "reversed":
        assert und == chain and (oi > oj).sum() == (P - 1) // 2 and (oi < oj).any()
    elif kind == "shuffled":
        assert und == chain and list(zip(oi.tolist(), oj.tolist())) != chain
    elif kind in ("long", "duplicate_long"):
        assert 2 <= len(far) <= 4, far                      # poses that share no landmark: only odometry couples them
    if kind.startswith("hub"):
        deg = np.bincount(np.r_[oi, oj], minlength=P)
        h = int(deg.argmax())
        nb = set(oj[oi == h].tolist()) | set(oi[oj == h].tolist())
        assert deg[h] == int(kind[3:]) == len(nb) and h not in nb and (oi == h).any() and (oj == h).any()
    if kind == "fixed_ends":
        f = np.asarray(g.fixed, bool)
        kinds = set(zip(f[oi].tolist(), f[oj].tolist()))
        assert {(True, False), (False, True), (True, True), (False, False)} <= kinds and f.sum() >= 3
    if kind in ("duplicate", "duplicate_long"):
        pairs = list(zip(oi.tolist(), oj.tolist()))
        assert dup and loops == 0
        assert any(pairs.count(p) == 2 for p in pairs)                        # one pair twice, same direction
        assert any(p[0] > p[1] and (p[1], p[0]) in pairs for p in pairs)      # and one as both (a, b) and (b, a)
    elif kind == "self_loop":
        k = int(np.nonzero(oi == oj)[0][0])
        assert loops == 1 and np.abs(g.o_meas[k]).max() > 0
    else:
        assert not dup and loops == 0


def odo_graph(synth, P, L, kind):
    g = synth.odometry_topology(synth.ba_graph(P, L), kind)
    assert_topology(synth, g, kind)
    return g


def _info_inputs(synth, P=12, L=200, seed=0, g=None):
    """Inputs of Map::loadLocalGraph's information computation (Map.cpp:1024-1049) for a synthetic window (g: that window, with
    its own camera, instead of synth.ba_graph(P, L))."""
    g = synth.ba_graph(P, L) if g is None else g
    rng = np.random.default_rng(seed)
    Rcb = g.Rbc.T
    tcb = -Rcb @ g.tbc
    _, _, _, lc = synth._project(g.poses, g.lms, g.e_kf, g.e_lm, Rcb, tcb, g.fx, 0.0, 0.0)
    th = g.poses[:, 2]
    Rbw = np.zeros((g.P, 3, 3))
    Rbw[:, 0, 0] = np.cos(th); Rbw[:, 0, 1] = np.sin(th); Rbw[:, 1, 0] = -np.sin(th); Rbw[:, 1, 1] = np.cos(th)
    Rbw[:, 2, 2] = 1
    Rcw = (Rcb[None] @ Rbw).astype(np.float32)
    level = rng.integers(0, 8, g.E)
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(1.2)
    sig2 = (sf * sf).astype(np.float32)
    return dict(lc=lc.astype(np.float32), lw=g.lms[g.e_lm].astype(np.float32), e_kf=g.e_kf, sigma2=sig2[level],
                Rcw=Rcw.reshape(g.P, 9), twb_xy=g.poses[:, :2].astype(np.float32), fx=np.float32(g.fx)), g, level


# ---- SE3 windows beyond ba3_graph's chain (synth.odometry_topology3) --------------------------------------------------------
def odometry_cases3(synth, sizes, kinds=None):
    """(P, L, n_ref, kind) of every SE3 odometry topology a window of that size can hold: a hub of N edges needs N + 1 local key
    frames, to_reference needs reference key frames, dense needs DENSE_TERMS - P distinct pairs"""
    out = []
    for P, L, n_ref in sizes:
        nL = P - n_ref
        for kind in (synth.ODOMETRY_TOPOLOGIES3 if kinds is None else kinds):
            if kind.startswith("hub") and int(kind[3:]) + 1 > nL:
                continue
            if kind == "to_reference" and n_ref == 0:
                continue
            if kind == "dense" and synth.DENSE_TERMS - P - (nL - 1) > nL * (nL - 1) // 2 - (nL - 1) + nL * n_ref:
                continue
            out.append((P, L, n_ref, kind))
    return out


def assert_topology3(synth, g, kind, base):
    """the odometry and the priors of `g` have the shape synth.odometry_topology3(base, kind) claims"""
    P, nL = g.P, synth.n_local(base)
    oi, oj = np.asarray(g.o_i, np.int64), np.asarray(g.o_j, np.int64)
    und = sorted(zip(np.minimum(oi, oj).tolist(), np.maximum(oi, oj).tolist()))
    chain = [(k, k + 1) for k in range(nL - 1)]
    assert len(set(und)) == len(und) and not (oi == oj).any()          # the SE3 call surface refuses duplicates and self loops
    assert g.o_meas.shape == (g.O, 4, 4) and g.o_info.shape == (g.O, 6, 6)
    if kind != "none":
        assert set(chain) <= set(und)
        assert np.linalg.eigvalsh(g.o_info).min() > 0
    if kind not in ("dense", "to_reference"):
        assert g.O == 0 or max(oi.max(), oj.max()) < nL                # pairs among the local key frames
    f = np.asarray(g.fixed, bool)
    if kind != "fixed_ends":
        assert np.array_equal(g.fixed, base.fixed)
    if kind != "sparse_priors":
        assert np.array_equal(g.has_prior, base.has_prior)
    cov = synth.covisible(g)
    if kind == "reversed":
        assert und == chain and (oi > oj).sum() == (nL - 1) // 2 and (oi < oj).any()
    elif kind == "shuffled":
        assert und == chain and list(zip(oi.tolist(), oj.tolist())) != chain
    elif kind == "long":
        far = [(i, j) for i, j in zip(oi, oj) if abs(i - j) >= 2]
        assert 2 <= len(far) <= 4 and not any(cov[i, j] for i, j in far)     # only the odometry edge couples these key frames
        assert any(i < j for i, j in far) and any(i > j for i, j in far)
    elif kind.startswith("hub"):
        deg = np.bincount(np.r_[oi, oj], minlength=P)
        h = int(deg.argmax())
        assert h == nL // 2 and deg[h] == int(kind[3:]) and (oi == h).sum() >= 2 and (oj == h).sum() >= 2
    elif kind == "dense":
        assert P + g.O == synth.DENSE_TERMS > 256
        assert (oi > oj).sum() > 20 and (oi < oj).sum() > 20
        assert (np.maximum(oi, oj) >= nL).any() == (nL < P) and np.minimum(oi, oj).max() < nL     # never reference to reference
    elif kind == "fixed_ends":
        kinds = set(zip(f[oi].tolist(), f[oj].tolist()))
        assert {(True, False), (False, True), (True, True), (False, False)} <= kinds
        assert f[[0, 1, nL // 2, nL - 1]].all() and f[:nL].sum() == 4 and np.array_equal(f[nL:], np.asarray(base.fixed, bool)[nL:])
        assert g.has_prior[[1, nL // 2, nL - 1]].all()                 # priors on fixed poses other than pose 0
    elif kind == "to_reference":
        ref = [(i, j) for i, j in zip(oi, oj) if max(i, j) >= nL]
        assert 2 <= len(ref) <= 4 and all(min(i, j) < nL for i, j in ref)
        assert any(i < j for i, j in ref) and any(i > j for i, j in ref)
    elif kind == "none":
        assert g.O == 0
    elif kind == "sparse_priors":
        assert und == chain
        free = ~f
        lost = free & (np.asarray(g.has_prior) == 0)
        assert lost.sum() == len(np.nonzero(free)[0][2::3]) > 0 and (free & (np.asarray(g.has_prior) == 1)).any()
        assert np.array_equal(np.asarray(g.has_prior)[f], np.asarray(base.has_prior)[f])


def odo_graph3(synth, P, L, n_ref, kind):
    base = synth.ba3_graph(P, L, n_ref)
    if kind == "chain":
        return base
    g = synth.odometry_topology3(base, kind)
    assert_topology3(synth, g, kind, base)
    return g


# ---- a landmark-sharded run on one device -----------------------------------------------------------------------------------
def sharded_equals_single(g, iters, trials=None, world=2, debug_lam=None, stop=None):
    """`world` landmark shards as `world` handles on `world` threads of ONE GPU; the all-reduce callback (no caller-owned
    buffer, so the library hands it the PACKED exchange: the lower-triangular tiles of [S; b^T], se2gpu_ba_exchange_doubles)
    sums the ranks' buffers on the host.  Same collective pattern as the RCCL path, which takes this buffer too.
    `stop`: a force-stop flag every handle polls (a raised one ends the runs before any system is exchanged).  Returns the single
    handle and the ranks' (stats, estimates)."""
    from se2lam_amd import capi
    from se2lam_amd.optimizer import SlamOptimizer
    single = opt(g)
    single.setForceStopFlag(stop)
    single.optimize(iters)
    if trials is not None:
        assert single.stats["trials_hist"] == trials
    # the packed exchange of the system the solver factorises: the ranks of a sharded run re-order the poses like the
    # single handle does (nested dissection from the merged block pattern), so its size comes from the handle
    packed = single.exchange_doubles()
    assert packed >= int(capi.lib().se2gpu_ba_exchange_doubles(g.P))      # = in the natural order, padded partitions otherwise
    rows = 3 * g.P + 1
    rect = rows * (-(-rows // 32) * 32)              # the rows of [S; b^T] the rectangular exchange would ship (ld = 32-padded)
    if packed == int(capi.lib().se2gpu_ba_exchange_doubles(g.P)):
        assert packed <= rect and (packed < rect or rows <= 32)   # the packed triangle is smaller from two tile rows on
    barrier = threading.Barrier(world)
    stage = [None] * world
    results = [None] * world
    dbg = [None] * world
    counts = [set() for _ in range(world)]
    errors = []

    def make_cb(rank):
        def cb(ptr, count, stream):
            counts[rank].add(int(count))
            capi.check(capi.lib().se2gpu_device_synchronize())
            buf = np.empty(count)
            capi.check(capi.lib().se2gpu_memcpy_d2h(capi.vp(buf), ptr, buf.nbytes))
            stage[rank] = buf
            barrier.wait()
            tot = stage[0].copy()                    # fixed summation order on every rank: bit-identical sums
            for r in range(1, world):
                tot += stage[r]
            barrier.wait()
            capi.check(capi.lib().se2gpu_memcpy_h2d(ptr, capi.vp(tot), tot.nbytes))
        return cb

    def run(rank):
        try:
            o = SlamOptimizer()
            o.set_shard(rank, world)
            o.set_allreduce(make_cb(rank))
            o.load(g.shard(rank, world))
            o.initializeOptimization(0)
            o.setForceStopFlag(stop)
            assert o.exchange_doubles() == packed     # every rank chose the single handle's order
            if debug_lam is not None:                 # the debug entry points are collectives too
                dbg[rank] = (o.reduced_system(debug_lam), o.solve(debug_lam))
            o.optimize(iters)
            assert o.solver_path() == 0
            results[rank] = (o.stats, o.estimates())
        except Exception as exc:  # pragma: no cover
            errors.append(exc)
            barrier.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for r in range(world):
        st, (poses, _) = results[r]
        assert st["trials_hist"] == single.stats["trials_hist"]
        assert np.allclose(st["chi2_hist"], single.stats["chi2_hist"], rtol=1e-9)
        assert np.allclose(st["lambda_hist"], single.stats["lambda_hist"], rtol=1e-9)
        assert np.allclose(poses, single.estimates()[0], rtol=1e-8, atol=1e-8)
        assert np.array_equal(poses, results[0][1][0])  # replicated poses stay bit-identical across the ranks
        # the system exchange went through the packed triangle (the other exchanges are 4 scalars / world slots / 3P diagonals)
        assert stop is not None or packed in counts[r] and (packed >= rect or debug_lam is not None or not any(c >= rect for c in counts[r])), sorted(counts[r])
    if debug_lam is not None:   # se2gpu_ba_debug_reduced_system / _solve on a sharded handle whose poses were re-ordered
        fresh = opt(g)
        S0, b0 = fresh.reduced_system(debug_lam)
        x0, ok0 = fresh.solve(debug_lam)
        assert ok0
        for r in range(world):
            (S, b), (x, ok) = dbg[r]
            assert ok and np.abs(S - S0).max() <= 1e-10 * np.abs(S0).max() and np.abs(b - b0).max() <= 1e-10 * np.abs(b0).max()
            assert np.abs(x - x0).max() <= 1e-8 * np.abs(x0).max()
            sp.close(S, b, S0, b0, 1e-10, ("shard", r, "against the single handle"))     # the same in the system's own scale
            assert sp.step_distance(x, x0, 3) <= 1e-8
    # every landmark lives on exactly one rank: the shards' landmark estimates together are the single run's
    lms = np.full_like(single.estimates()[1], np.nan)
    for r in range(world):
        own = g.shard_landmarks(r, world)
        lms[own] = results[r][1][1]
    assert np.allclose(lms, single.estimates()[1], rtol=1e-8, atol=1e-6)
    return single, results
