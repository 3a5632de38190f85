"""The one-workgroup-per-window path of se2gpu_ba_optimize_batch for SE3-expmap windows (csrc/ba_window3.hip, pose model 1:
Map::loadLocalGraph + LocalMapper::removeOutlierChi2 with EdgeProjectXYZ2UV, EdgeSE3ExpmapPrior and EdgeSE3Expmap).  Sums into the
reduced system are LDS atomics (no fixed order), so the path is held to the multi-launch k3_* path and to the oracle trial for trial
and to 1e-9 on costs, poses and landmarks - not bit for bit.  Paths that do not take a batch stay bit-identical to one-by-one runs."""
import copy
import functools

import numpy as np
import pytest

from se2lam_amd import synth as _synth            # (for a parametrisation; tests take the `synth` fixture)
from ba_cases import REJECT, env, kidnapped3, multi_launch, odo_graph3, odometry_cases3, opt, opt3

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def _last_path():
    from se2lam_amd import capi
    return int(capi.lib().se2gpu_ba_last_batch_path())


def _edge_chi2(o, g):
    from se2lam_amd import optimizer as op
    return op.edgeChi2(o, g.E)


_multi_launch = functools.partial(multi_launch, make=opt3)


def _same(o, ref, what, g=None):
    st, est, ec = ref
    n = st["iterations"]
    assert o.stats["iterations"] == n and o.stats["trials"] == st["trials"], what
    assert o.stats["trials_hist"] == st["trials_hist"], (what, o.stats["trials_hist"], st["trials_hist"])
    assert o.stats["terminated"] == st["terminated"] and o.stats["stopped"] == st["stopped"], what
    assert np.isclose(o.stats["chi2_init"], st["chi2_init"], rtol=RTOL), what
    assert np.allclose(o.stats["chi2_hist"][:n], st["chi2_hist"][:n], rtol=RTOL), what
    assert np.allclose(o.stats["lambda_hist"][:n], st["lambda_hist"][:n], rtol=1e-7), what
    p, l = o.estimates()
    assert np.allclose(p, est[0], rtol=1e-9, atol=1e-9) and np.allclose(l, est[1], rtol=1e-9, atol=1e-7), what
    if g is not None and ec is not None:
        fixed = np.asarray(g.fixed, bool)
        assert np.array_equal(p[fixed], est[0][fixed]), what                    # fixed poses: to the bit
        got = _edge_chi2(o, g)
        assert np.allclose(got, ec, rtol=1e-6, atol=1e-9), what
        assert np.array_equal(got > 25, ec > 25), what                          # removeOutlierChi2's list


def _renumber(g, e_kf, e_lm):
    keep = np.unique(e_lm)                       # landmarks that lost all their observations leave the graph
    renum = np.full(g.L, -1, np.int64)
    renum[keep] = np.arange(len(keep))
    e_lm = renum[e_lm]
    order = np.argsort(e_lm, kind="stable")
    g.lms = np.asarray(g.lms)[keep].copy()
    g.e_kf, g.e_lm = e_kf[order].astype(np.int32), e_lm[order].astype(np.int32)
    g.e_uv, g.e_w = np.asarray(g.e_uv)[order].copy(), np.asarray(g.e_w)[order].copy()
    return g


def _merged3(synth, P=26, L=700, groups=10, per_group=4):
    """landmarks with 9 to 64 observations (the 16-lane and wave-per-landmark classes): up to `per_group` landmarks whose observers
    do not overlap are fused into one (as tests/ba_cases.py, merged_landmarks)"""
    g = copy.copy(synth.ba3_graph(P, L, 0))
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
        if len(members) > 1:
            used.update(members)
            for b in members[1:]:
                e_lm[e_lm == b] = a
            fused += 1
    return _renumber(g, e_kf, e_lm)


def _wide3(synth, k, P=70, L=1500, n_ref=50):
    """a window of P key frames, the last n_ref of them fixed reference key frames (so that the free ones fit a compute unit's LDS),
    in which landmark 0 has exactly k observations: observations of other landmarks by key frames it is not yet seen from move to it"""
    g = copy.copy(synth.ba3_graph(P, L, n_ref))
    e_kf, e_lm = np.asarray(g.e_kf).copy(), np.asarray(g.e_lm).copy()
    seen = set(e_kf[e_lm == 0].tolist())
    for b in range(1, g.L):
        if len(seen) >= k:
            break
        for t in np.nonzero(e_lm == b)[0]:
            if len(seen) < k and int(e_kf[t]) not in seen:
                seen.add(int(e_kf[t]))
                e_lm[t] = 0
    assert len(seen) == k
    g = _renumber(g, e_kf, e_lm)
    cnt = np.bincount(g.e_lm, minlength=g.L)
    assert cnt.max() == k and int((cnt == k).sum()) == 1
    return g


def _forced_graphs(synth):
    return [synth.ba3_graph(8, 60, 0), synth.ba3_graph(21, 800, 0), synth.ba3_graph(21, 800, 4), synth.ba3_graph(30, 2000, 6),
            kidnapped3(synth, *REJECT), _merged3(synth)]


def test_forced_se3_batch_equals_multi_launch_and_the_oracle(oracle, synth):
    from se2lam_amd.optimizer import optimize_batch
    graphs = _forced_graphs(synth)
    assert int(np.asarray(graphs[3].fixed).sum()) == 6 and graphs[3].P - 6 == 24                 # 24 free key frames
    kmax = np.bincount(np.asarray(graphs[5].e_lm)).max()
    cnt = np.bincount(np.asarray(graphs[5].e_lm))
    assert kmax > 16 and ((cnt > 8) & (cnt <= 16)).any(), kmax                                # 16-lane and whole-wave classes
    ref = [_multi_launch(g, 10) for g in graphs]
    assert max(ref[4][0]["trials_hist"]) > 1, ref[4][0]["trials_hist"]                        # the kidnapped start rejects trials
    opts = [opt3(g) for g in graphs]
    with env(SE2GPU_BA_RESIDENT="1"):
        its = optimize_batch(opts, 10)
    assert _last_path() == 2
    for g, o, r, n in zip(graphs, opts, ref, its):
        assert n == r[0]["iterations"]
        _same(o, r, (g.P, g.L, g.E), g)
    for g, o in zip(graphs[:5], opts[:5]):
        p_ref, l_ref, ec_ref, st = oracle.ba3_optimize(g, 10)
        assert o.stats["trials_hist"] == st["trials_hist"], (g.P, g.L)
        assert np.allclose(o.stats["chi2_hist"][:10], st["chi2_hist"][:10], rtol=1e-7)


def test_se3_modes_repeats_and_the_stop_flag(synth):
    from se2lam_amd.optimizer import optimize_batch, reset_estimates_batch
    graphs = [synth.ba3_graph(8, 60, 0), synth.ba3_graph(21, 800, 4), kidnapped3(synth, *REJECT)]
    opts = [opt3(g) for g in graphs]
    with env(SE2GPU_BA_RESIDENT="1"):
        for mode, iters in ((0, 10), (1, 10), (0, 4), (0, 0)):
            ref = [_multi_launch(g, iters, mode) for g in graphs]
            for rep in range(2):                   # the second run starts from the reset estimates on the same handles
                reset_estimates_batch(opts)
                optimize_batch(opts, iters, mode)
                assert _last_path() == 2
                for g, o, r in zip(graphs, opts, ref):
                    if mode == 1:   # undamped Gauss-Newton amplifies the last bits of every sum: its first steps only
                        assert np.allclose(o.stats["chi2_hist"][:3], r[0]["chi2_hist"][:3], rtol=1e-8), (g.P, g.L)
                        continue
                    _same(o, r, (g.P, g.L, mode, iters, rep), g)
        stop = np.ones(1, np.uint8)
        reset_estimates_batch(opts)
        its = optimize_batch(opts, 10, 0, stop)
        assert its == [0] * len(opts) and all(o.stats["stopped"] for o in opts)
        assert all(np.isclose(o.stats["chi2_final"], o.stats["chi2_init"]) for o in opts)


def _without(g, drop):
    """the window without the edges `drop` (removeOutlierChi2 moves them to level 1: the next optimize() does not see them)"""
    h = copy.copy(g)
    keep = ~drop
    h.e_kf, h.e_lm = np.asarray(g.e_kf)[keep], np.asarray(g.e_lm)[keep]
    h.e_uv, h.e_w = np.asarray(g.e_uv)[keep], np.asarray(g.e_w)[keep]
    return h


def test_se3_outlier_flow(synth):
    """LocalMapper::removeOutlierChi2: optimize, drop the edges whose chi2() exceeds 25, re-initialise, optimize again - both
    batches resident, equal to the same flow on the multi-launch path"""
    from se2lam_amd.optimizer import optimize_batch
    graphs = [synth.ba3_graph(21, 800, 4), kidnapped3(synth, *REJECT), synth.ba3_graph(30, 2000, 6)]
    ref1 = [_multi_launch(g, 5) for g in graphs]
    second = [_without(g, r[2] > 25) for g, r in zip(graphs, ref1)]
    assert sum(int((r[2] > 25).sum()) for r in ref1) > 0
    ref2 = [_multi_launch(g, 10) for g in second]
    with env(SE2GPU_BA_RESIDENT="1"):
        opts = [opt3(g) for g in graphs]
        optimize_batch(opts, 5)
        assert _last_path() == 2
        for g, o, r in zip(graphs, opts, ref1):
            _same(o, r, ("first", g.P), g)
            assert np.array_equal(_edge_chi2(o, g) > 25, r[2] > 25)
        opts = [opt3(g) for g in second]
        optimize_batch(opts, 10)
        assert _last_path() == 2
        for g, o, r in zip(second, opts, ref2):
            _same(o, r, ("second", g.P, g.E), g)


def test_mixed_se2_and_se3_batch(synth):
    from se2lam_amd.optimizer import optimize_batch
    g2 = [synth.ba_graph(8, 60), synth.ba_graph(21, 800), synth.ba_graph(50, 5000)]
    g3 = [synth.ba3_graph(8, 60, 0), synth.ba3_graph(21, 800, 4), synth.ba3_graph(30, 2000, 6)]
    ref = [_multi_launch(g, 8, make=opt) for g in g2] + [_multi_launch(g, 8) for g in g3]
    opts = [opt(g) for g in g2] + [opt3(g) for g in g3]
    order = [0, 3, 1, 4, 2, 5]                     # interleaved in the call
    with env(SE2GPU_BA_RESIDENT="1"):
        optimize_batch([opts[i] for i in order], 8)
    assert _last_path() == 2
    for i, (o, r) in enumerate(zip(opts, ref)):
        _same(o, r, i, g3[i - 3] if i >= 3 else None)


def test_se3_windows_too_large_or_too_wide(oracle, synth):
    """49 free key frames do not fit a compute unit's LDS: the batch stays off the resident path, bit-identical to one-by-one runs.
    A landmark of 65 observations is refused by the kernel and its window run on the multi-launch path; one of 64 stays resident."""
    from se2lam_amd.optimizer import optimize_batch
    graphs = [synth.ba3_graph(8, 60, 0), synth.ba3_graph(50, 5000, 0)]
    ref = [_multi_launch(g, 6) for g in graphs]
    opts = [opt3(g) for g in graphs]
    with env(SE2GPU_BA_RESIDENT="1"):
        optimize_batch(opts, 6)
    assert _last_path() != 2
    for o, (st, est, _) in zip(opts, ref):
        assert o.stats == st and np.array_equal(o.estimates()[0], est[0]) and np.array_equal(o.estimates()[1], est[1])
    small = synth.ba3_graph(21, 800, 0)
    for k in (65, 64):
        wide = _wide3(synth, k)
        ref = [_multi_launch(g, 8) for g in (small, wide)]
        opts = [opt3(small), opt3(wide)]
        with env(SE2GPU_BA_RESIDENT="1"):
            optimize_batch(opts, 8)
        assert _last_path() == 2
        _same(opts[0], ref[0], ("ordinary window next to", k), small)
        if k == 65:
            st, est, _ = ref[1]
            assert opts[1].stats == st
            assert np.array_equal(opts[1].estimates()[0], est[0]) and np.array_equal(opts[1].estimates()[1], est[1])
        else:
            _same(opts[1], ref[1], k, wide)


def test_se3_default_threshold(synth):
    """without the switch, 95 SE3 windows stay on the multi-launch path (bit-identical to one-by-one runs); 96 take the resident one"""
    from se2lam_amd.optimizer import optimize_batch
    g = synth.ba3_graph(8, 60, 0)
    ref = _multi_launch(g, 6)
    with env(SE2GPU_BA_RESIDENT=None):
        small = [opt3(g) for _ in range(95)]
        optimize_batch(small, 6)
        assert _last_path() != 2
        for o in small:
            assert o.stats == ref[0] and np.array_equal(o.estimates()[0], ref[1][0]) and np.array_equal(o.estimates()[1], ref[1][1])
        del small
        large = [opt3(g) for _ in range(96)]
        optimize_batch(large, 6)
        assert _last_path() == 2
        for o in large[::8]:
            _same(o, ref, "96 windows", g)


# ---- SE3 windows beyond ba3_graph's chain (synth.odometry_topology3) on the resident kernel: odometry_term's two tri() arms
# (edges stored as (i > j)), blocks only an odometry edge fills, pose_terms' stride once P + O exceeds the workgroup (`dense`),
# fixed ends and reference key frames, no odometry at all, free key frames without a prior
RESIDENT_SIZES3 = ((8, 60, 0), (21, 800, 0), (21, 800, 4))                  # at most 27 free key frames: the 256-thread width
KIDNAP_REVERSED_LONG = (21, 800, 0, 3000.0, 0.8, 2, 8)   # the oracle (picked with it, once): trials [1, 1, 1, 5, 1, 3, 1, 4, 1, 1],
                                                         # the closest gain ratio 7.8e-3 from zero


def _kidnapped_reversed_long(synth):
    """a kidnapped start under the `reversed` chain plus the `long` kind's extra edges: rejected trials re-evaluate edges stored as
    (i > j) and edges between key frames without a common landmark"""
    k = kidnapped3(synth, *KIDNAP_REVERSED_LONG)
    rv, lg = synth.odometry_topology3(k, "reversed"), synth.odometry_topology3(k, "long")
    extra = list(zip(lg.o_i[rv.O:].tolist(), lg.o_j[rv.O:].tolist()))
    cov = synth.covisible(k)
    assert len(extra) >= 2 and not any(cov[i, j] for i, j in extra) and any(i > j for i, j in extra)
    g = synth.with_odometry3(k, list(zip(rv.o_i.tolist(), rv.o_j.tolist())) + extra)
    assert (g.o_i > g.o_j).sum() >= 10
    return g


def _resident_cases3(synth, kind):
    """the windows of `kind` that fit the resident kernel: RESIDENT_SIZES3, and 20 local + 50 reference key frames for to_reference
    and dense"""
    cases = odometry_cases3(synth, RESIDENT_SIZES3, (kind,)) + odometry_cases3(synth, ((70, 1500, 50),), (kind,) if kind in ("to_reference", "dense") else ())
    assert cases, kind                                                       # every kind fits somewhere
    return [(c, odo_graph3(synth, *c)) for c in cases]


@pytest.mark.parametrize("kind", _synth.ODOMETRY_TOPOLOGIES3 + ("kidnapped",))
def test_forced_se3_odometry_topologies_equal_multi_launch_and_the_oracle(oracle, synth, kind):
    """one forced batch per layout (every size of it that fits, and for "kidnapped" a start that rejects trials under reversed and
    long edges): test_forced_se3_batch_equals_multi_launch_and_the_oracle's checks"""
    from se2lam_amd.optimizer import optimize_batch
    if kind == "kidnapped":
        cases = [("kidnapped, reversed + long", _kidnapped_reversed_long(synth))]
    else:
        cases = _resident_cases3(synth, kind)
    graphs = [g for _, g in cases]
    if kind == "dense":
        assert all(g.P + g.O > 256 and int((np.asarray(g.fixed) == 0).sum()) <= 27 for g in graphs)   # pose_terms strides at 256 threads
    ref = [_multi_launch(g, 10) for g in graphs]
    if kind == "kidnapped":
        assert max(ref[0][0]["trials_hist"]) > 1, ref[0][0]["trials_hist"]                    # the kidnapped start rejects trials
    opts = [opt3(g) for g in graphs]
    with env(SE2GPU_BA_RESIDENT="1"):
        its = optimize_batch(opts, 10)
    assert _last_path() == 2
    for (c, g), o, r, n in zip(cases, opts, ref, its):
        assert n == r[0]["iterations"], c
        _same(o, r, c, g)
        p_ref, l_ref, ec_ref, st = oracle.ba3_optimize(g, 10)
        assert o.stats["trials_hist"] == st["trials_hist"], c
        assert np.allclose(o.stats["chi2_hist"][:10], st["chi2_hist"][:10], rtol=1e-7), c


def _lds3_bytes(P, nfree, threads):
    """ba_window3_lds_bytes (csrc/ba_window3.hip: window_lds_bytes of csrc/ba_window_skeleton.h with the SE3 model's constants) restated by reading it, not from a run: dynamic LDS = the column list (P ints), two
    sets of poses (12 doubles each per key frame of the window, fixed ones included), x and 1 / diag (6 nfree each), the staging
    strip (19 doubles per thread) and the packed triangle of S with b_s and a zero block row ((n + 6)(n + 7) / 2), n = 6 nfree;
    static LDS = BaCtl (1392 bytes) + the histogram, wave totals and lists (232 ints) + 45 doubles + 128; 160 KiB in all, n <= 192.
    -> bytes, 0 when the window does not fit"""
    if threads not in (256, 128):
        return 0
    n = 6 * nfree
    doubles = (P + 1) // 2 + 24 * P + 2 * n + threads * 19 + (n + 6) * (n + 7) // 2
    fixed = 1392 + (64 + 2 + 18 * 8 + 18 + 4) * 4 + (24 + 21) * 8 + 128
    return 0 if n > 192 or doubles * 8 + fixed > 160 * 1024 else doubles * 8


def _lds3_threads(g):
    nfree = int((np.asarray(g.fixed) == 0).sum())
    return next((t for t in (256, 128) if _lds3_bytes(g.P, nfree, t)), 0)


def _limit_windows(synth):
    """windows of 27, 28, 29 and 30 free key frames with 2 reference key frames each (P = 29 .. 32).  By _lds3_bytes at these P: 27
    free take the 256-thread workgroup, 28 and 29 only the 128-thread one, 30 none - the limits the kernel's commit states.  (They
    move with P: 24 doubles per key frame of the window.  27 free fit 256 threads up to P = 30, 29 free fit 128 up to P = 43.)
    Each in another layout; `dense` strides pose_terms at 128 threads too."""
    out = []
    for nfree, kind, threads in ((27, "reversed", 256), (28, "dense", 128), (29, "long", 128), (30, "hub9", 0)):
        g = synth.odometry_topology3(synth.ba3_graph(nfree + 2, 600, 2), kind)
        assert int((np.asarray(g.fixed) == 0).sum()) == nfree and g.P == nfree + 2
        assert _lds3_threads(g) == threads, (nfree, g.P, _lds3_threads(g))                  # up front: the intended side of each limit
        out.append(g)
    assert out[1].P + out[1].O > 256
    return out


def test_se3_lds_limits(synth):
    """on either side of the two LDS limits of k_window_lm3: forced, 27 / 28 / 29 free key frames run resident (one launch of 256
    threads, one of 128) and equal the multi-launch run; with a 30-free window the batch stays off the resident path, bit-identical
    to one-by-one runs; unforced, one 28-free window keeps a batch of 96 off it (the t < 256 rule)"""
    from se2lam_amd.optimizer import optimize_batch
    w27, w28, w29, w30 = _limit_windows(synth)
    ref = [_multi_launch(g, 8) for g in (w27, w28, w29, w30)]
    opts = [opt3(g) for g in (w27, w28, w29)]
    with env(SE2GPU_BA_RESIDENT="1"):
        optimize_batch(opts, 8)
    assert _last_path() == 2
    for g, o, r in zip((w27, w28, w29), opts, ref):
        _same(o, r, ("free", g.P - 2), g)
    opts = [opt3(g) for g in (w27, w30)]
    with env(SE2GPU_BA_RESIDENT="1"):
        optimize_batch(opts, 8)
    assert _last_path() != 2
    for o, (st, est, _) in zip(opts, (ref[0], ref[3])):
        assert o.stats == st and np.array_equal(o.estimates()[0], est[0]) and np.array_equal(o.estimates()[1], est[1])
    small = synth.odometry_topology3(synth.ba3_graph(8, 60, 0), "reversed")
    rs = _multi_launch(small, 8)
    with env(SE2GPU_BA_RESIDENT=None):
        opts = [opt3(small) for _ in range(95)] + [opt3(w28)]
        optimize_batch(opts, 8)
        assert _last_path() != 2
        for o in opts[:3]:
            assert o.stats == rs[0] and np.array_equal(o.estimates()[0], rs[1][0])
        assert opts[-1].stats == ref[1][0] and np.array_equal(opts[-1].estimates()[0], ref[1][1][0])
        del opts
        opts = [opt3(small) for _ in range(95)] + [opt3(w27)]               # (with a 27-free window instead the batch goes resident)
        optimize_batch(opts, 8)
        assert _last_path() == 2
        _same(opts[-1], ref[0], "27 free among 96", w27)
        _same(opts[0], rs, "8 key frames among 96", small)
