"""csrc/se3_math.h on the device, function by function (se2gpu_debug_se3: one function per thread, one launch per op, compiled
with the flags of ba.hip / ba_window3.hip), against tests/se3_mp.py: the same formulas and the exact exponential / logarithm in
mpmath at 50 digits.  About 2,000 inputs, among them the branch thresholds one ulp either side, angles near pi, the three
non-positive-trace quaternion cases with their ties, float32-rounded matrices and compact quaternions on both sides of |q| = 1.

Bounds (none is taken from what the device gives):
  exp, log, mul   per input group, relative to the largest entry of the output block (rotation / translation, omega / upsilon):
                  4 x the largest distance of the oracle's host evaluation (oracle/se3_ref.h through oracle.se3_exp / se3_log /
                  se3_mul) from mpmath on the same inputs - the factor for contraction and another libm - and at least 16 ulp.
  straight-line   (normalize_rotation, quat_of, to_mqt, from_mqt, se3_adj, mqt_jac_*): 64 ulp of the largest operand, from counting
                  operations: the longest chain is quat_of -> product of two quaternions -> sum of four products, under 30 roundings.
  conditioning    se3_log divides by sqrt(1 - d^2) = sin(theta): an error eps in d moves it by eps d / sin(theta), relative
                  eps / (pi - theta)^2 near pi, so a bound is scaled by max(1, 1 / (pi - theta)^2).  from_mqt takes sqrt(w) of
                  w = 1 - |q|^2, whose sum carries an ulp of 1: d sqrt(w) = dw / (2 sqrt(w)), scale max(1, 1 / sqrt(w)).
  truncation      against the EXACT maps, where g2o's small-angle branches are not exact:
                  exp, theta < 1e-5: R = normalise(I + Om + Om^2) against I + a Om + b Om^2, a = 1 - theta^2/6.., b = 1/2 - ..:
                    the symmetric part is off by theta^2/2 and the antisymmetric by theta^3/6: |dR| <= theta^2;  V = I + Om + Om^2
                    against I + Om/2 + Om^2/6..: |dt| <= (theta/2 + theta^2) |upsilon| - first order, g2o's own "TODO: check";
                  log, d > 0.99999 (theta < 4.5 mrad): omega = (R - R')^v / 2 = (sin theta / theta) omega_exact:
                    |d omega| <= theta^3/6;  V^-1 = I - Om'/2 + Om'^2/12 with that omega against I - Om/2 + (1/12 + theta^2/720) Om^2:
                    |d upsilon| <= (theta^3/12)(1 + theta) |t|.
`python tests/test_se3_device_gpu.py FILE` writes the measured distances and the bounds as profiles/se3_device.md has them."""
import math
import sys

import numpy as np
import pytest

import se3_mp as M

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -52
FLOOR, FACTOR, STRAIGHT = 16, 4, 64
RECORD = {}          # op / group -> figures, for the record file


def _device(op, X):
    from se2lam_amd import capi
    return capi.debug_se3(op, X)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _axes(rng, n):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1)[:, None]


def _round_pose(T):
    return np.array(M.flat(T[0], T[1]))


def _f32(p12):
    p = np.array(p12, np.float64)
    p[:9] = p[:9].astype(np.float32).astype(np.float64)
    return p


def exp_inputs():
    """group -> (n, 6): (omega, upsilon), upsilon ~ N(0, 300 mm)"""
    rng = np.random.default_rng(20240601)
    ups = lambda n: rng.normal(0, 300.0, (n, 3))
    below, above = np.nextafter(M.THETA_SMALL, 0.0), np.nextafter(M.THETA_SMALL, 1.0)
    single = lambda th: np.concatenate([s * th * np.eye(3) for s in (1, -1)])
    g = {}
    g["theta 1e-5 - 1 ulp, one axis"] = np.c_[single(below), ups(6)]
    g["theta 1e-5 and + 1 ulp, one axis"] = np.c_[np.concatenate([single(M.THETA_SMALL), single(above)]), ups(12)]
    g["theta 1e-5 (1 - 1e-9)"] = np.c_[M.THETA_SMALL * (1 - 1e-9) * _axes(rng, 12), ups(12)]
    g["theta 1e-5 (1 + 1e-9)"] = np.c_[M.THETA_SMALL * (1 + 1e-9) * _axes(rng, 12), ups(12)]
    for th in (0.0, 1e-9, 1e-6):
        g["theta %g" % th] = np.c_[th * _axes(rng, 8), ups(8)]
    for th in (2e-5, 1e-4, 1e-3, 0.1, 1.0, 2.0, 3.0):
        g["theta %g" % th] = np.c_[th * _axes(rng, 24), ups(24)]
    for gap in (1e-3, 1e-6):
        g["theta pi - %g" % gap] = np.c_[(math.pi - gap) * _axes(rng, 16), ups(16)]
    return g


def log_inputs():
    """group -> (n, 12) poses: the exact exponential of the exp inputs rounded to double, the d threshold, float32 matrices"""
    g = {}
    for name, U in exp_inputs().items():
        if "ulp" in name or "1e-9)" in name:
            continue
        g[name] = np.stack([_round_pose(M.exp_exact(M.vec(u))) for u in U])
    rng = np.random.default_rng(20240602)
    rows = []
    for k in (-3, -2, -1, 0, 1, 2, 3):                       # rotations about z with cos = 0.99999 + k ulp: d = cos up to the
        c = M.D_SMALL                                         # rounding of (2 c + 1) - 1, so both sides of the threshold occur
        for _ in range(abs(k)):
            c = np.nextafter(c, 2.0 if k > 0 else 0.0)
        s = float(M.mp.sqrt(1 - M.F(c) ** 2))
        for sg in (1, -1):
            rows.append(np.r_[c, -sg * s, 0, sg * s, c, 0, 0, 0, 1, rng.normal(0, 300.0, 3)])
    g["d 0.99999 +- 3 ulp, about z"] = np.stack(rows)
    th0 = math.acos(M.D_SMALL)
    for f, tag in ((1 - 1e-6, "-"), (1 + 1e-6, "+")):
        U = np.c_[th0 * f * _axes(rng, 12), rng.normal(0, 300.0, (12, 3))]
        g["theta acos(0.99999) (1 %s 1e-6)" % tag] = np.stack([_round_pose(M.exp_exact(M.vec(u))) for u in U])
    U = np.c_[rng.uniform(0.01, 3.0, (30, 1)) * _axes(rng, 30), rng.normal(0, 300.0, (30, 3))]
    g["float32 matrices"] = np.stack([_f32(_round_pose(M.exp_exact(M.vec(u)))) for u in U])
    return g


def rotations():
    """group -> (n, 9): what quat_of / normalize_rotation meet"""
    rng = np.random.default_rng(20240603)
    R_of = lambda w: np.array(M.flat(M.exp_exact(M.vec(np.r_[w, 0, 0, 0]))[0]))
    g = {"random": np.stack([R_of(th * a) for th, a in zip(rng.uniform(0, math.pi, 60), _axes(rng, 60))])}
    for k in range(3):       # trace <= 0 with diagonal entry k the largest: 2.6 - 3.1 rad about an axis near e_k
        ax = np.eye(3)[k] + 0.25 * rng.normal(size=(24, 3))
        ax /= np.linalg.norm(ax, axis=1)[:, None]
        g["trace <= 0, R%d%d largest" % (k, k)] = np.stack([R_of(th * a) for th, a in zip(rng.uniform(2.6, 3.1, 24), ax)])
    ties = []
    for n in ([1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1], [-1, 1, 0], [-1, 0, 1], [0, -1, 1],
              [1, 1, 1], [1, -1, 1], [1, 1, -1], [1, -1, -1], [-1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]):
        n = np.array(n, float)
        ties.append((2 * np.outer(n, n) / (n @ n) - np.eye(3)).reshape(9))            # half a turn: symmetric to the bit, w = 0
    g["half turns with equal diagonal entries"] = np.stack(ties)
    g["float32 matrices"] = np.stack([R_of(th * a) for th, a in zip(rng.uniform(0, math.pi, 40), _axes(rng, 40))]).astype(np.float32).astype(np.float64)
    return g


def poses(seed, n, f32=0, least=0.0):
    """n poses turned by least..pi rad about random axes, translations ~ N(0, 2 m); the first f32 with float32 rotations"""
    rng = np.random.default_rng(seed)
    U = np.c_[rng.uniform(least, math.pi, (n, 1)) * _axes(rng, n), rng.normal(0, 2000.0, (n, 3))]
    P = np.stack([_round_pose(M.exp_exact(M.vec(u))) for u in U])
    for i in range(f32):
        P[i] = _f32(P[i])
    return P


def mqt_inputs():
    rng = np.random.default_rng(20240604)
    t = lambda n: rng.normal(0, 2000.0, (n, 3))
    g = {"|q| < 1": np.c_[t(60), rng.uniform(0, 0.999, (60, 1)) * _axes(rng, 60)]}
    g["|q| = 1 - 1e-12"] = np.c_[t(12), (1 - 1e-12) * _axes(rng, 12)]
    g["|q| = 1 + 1e-12"] = np.c_[t(12), (1 + 1e-12) * _axes(rng, 12)]
    one = lambda v: np.concatenate([s * v * np.eye(3) for s in (1, -1)])
    g["|q| = 1 - 1 ulp, one axis"] = np.c_[t(6), one(np.nextafter(1.0, 0.0))]
    g["|q| = 1 and 1 + 1 ulp, one axis"] = np.c_[t(12), np.concatenate([one(1.0), one(np.nextafter(1.0, 2.0))])]
    g["|q| small"] = np.c_[t(12), 1e-9 * _axes(rng, 12)]
    return g


def pairs():
    """(A, B): 90 pairs of any angle (the first 20 with float32 rotations) and 60 of more than 2.2 rad each, whose product turns by
    more than pi about half of the time: wprod of both signs"""
    A = np.concatenate([poses(20240605, 90, f32=20), poses(20240615, 60, least=2.2)])
    B = np.concatenate([poses(20240606, 90, f32=20), poses(20240616, 60, least=2.2)])
    return np.c_[A, B]


# ---- distances -------------------------------------------------------------------------------------------------------------------
def _rel(dev, ref, blocks):
    """per block: max |dev - ref| over the block / its largest |ref| (1 for a block that is zero)"""
    out = []
    for a, b in blocks:
        d = max(abs(M.F(float(x)) - r) for x, r in zip(dev[a:b], ref[a:b]))
        s = max(abs(r) for r in ref[a:b])
        out.append(float(d / (s if s else 1)))
    return out


def _abs(dev, ref):
    return float(max(abs(M.F(float(x)) - r) for x, r in zip(dev, ref)))


POSE_BLOCKS, TWIST_BLOCKS = ((0, 9), (9, 12)), ((0, 3), (3, 6))


def _theta_of(R):
    return float(M.mp.atan2(M.mp.sqrt((R[7] - R[5]) ** 2 + (R[2] - R[6]) ** 2 + (R[3] - R[1]) ** 2) / 2, (R[0] + R[4] + R[8] - 1) / 2))


def _log_cond(p12):
    th = _theta_of(M.pose(p12)[0])
    return max(1.0, 1.0 / (math.pi - th) ** 2)


def _against_oracle(op, groups, formula, oracle_fn, blocks, cond=lambda x: 1.0):
    """exp / log / mul: per group the device's and the oracle's distance from the 50-digit evaluation of the same formula, both
    divided by the input's conditioning; the bound is FACTOR x the oracle's largest, at least FLOOR ulp"""
    X = np.concatenate(list(groups.values()))
    dev = _device(op, X)
    worst, k = [], 0
    for name, G in groups.items():
        d_dev = d_or = 0.0
        for x in G:
            ref = formula(x)
            c = cond(x)
            d_dev = max(d_dev, max(_rel(dev[k], ref, blocks)) / c)
            d_or = max(d_or, max(_rel(oracle_fn(x), ref, blocks)) / c)
            k += 1
        bound = max(FACTOR * d_or, FLOOR * ULP)
        RECORD[(op, name)] = (len(G), d_or, d_dev, bound)
        print("%-4s %-36s n %3d  oracle %.2e  device %.2e  bound %.2e" % (op, name, len(G), d_or, d_dev, bound))
        worst.append((d_dev <= bound, name, d_dev, bound))
    return dev, X, worst


def _p12(T44):
    return np.r_[np.asarray(T44)[:3, :3].reshape(-1), np.asarray(T44)[:3, 3]]


def _T44(p12):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(p12[:9]).reshape(3, 3), p12[9:12]
    return T


# ---- exp -------------------------------------------------------------------------------------------------------------------------
def test_exp_same_formula_branch_and_exact_map(oracle):
    groups = exp_inputs()
    dev, X, worst = _against_oracle("exp", groups, lambda u: (lambda T: T[0] + T[1])(M.se3_exp(M.vec(u))),
                                    lambda u: _p12(oracle.se3_exp(u)), POSE_BLOCKS)
    taken = {True: 0, False: 0}
    k = 0
    for name, G in groups.items():
        B = RECORD[("exp", name)][3]                 # the device is within B of the formula, the formula within its truncation of exp
        for x in G:
            y, u = dev[k], M.vec(x)
            k += 1
            small = M.branch_exp(x)
            # the branch the device took: its translation lies next to one of the two formulas' (they differ by theta |upsilon| / 2)
            cand = {b: M.se3_exp(u, small=b)[1] for b in (True, False)} if np.any(x[:3]) else None       # (theta = 0: one formula)
            if cand and _abs(M.flat(cand[True]), cand[False]) > 1e4 * np.spacing(np.abs(x[3:]).max()):
                near = min(cand, key=lambda b: _abs(y[9:], cand[b]))
                assert near == small, (name, x, near, small)
                taken[small] += 1
            th, nu = float(M.mp.sqrt(sum(v * v for v in u[:3]))), float(np.linalg.norm(x[3:]))
            E = M.exp_exact(u)
            tol_R = (th * th if small else 0.0) + B
            tol_t = ((0.5 * th + th * th) * nu if small else 0.0) + B * float(max(abs(v) for v in E[1]))
            assert _abs(y[:9], E[0]) <= tol_R, (name, x, _abs(y[:9], E[0]), tol_R)
            assert _abs(y[9:], E[1]) <= tol_t, (name, x, _abs(y[9:], E[1]), tol_t)
    assert taken[True] >= 20 and taken[False] >= 100, taken
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]


# ---- log -------------------------------------------------------------------------------------------------------------------------
def test_log_same_formula_branch_and_exact_map(oracle):
    groups = log_inputs()
    dev, X, worst = _against_oracle("log", groups, lambda p: M.se3_log(M.pose(p)), lambda p: oracle.se3_log(_T44(p)), TWIST_BLOCKS,
                                    cond=_log_cond)
    taken = {True: 0, False: 0}
    thr = groups["d 0.99999 +- 3 ulp, about z"]
    sides = {M.branch_log(p[:9]) for p in thr}
    assert sides == {True, False}                                    # the threshold group lies on both sides, in double
    assert any(abs(M.d_double(p[:9]) - M.D_SMALL) <= np.spacing(M.D_SMALL) for p in thr)
    k = 0
    for name, G in groups.items():
        for x in G:
            y, T = dev[k], M.pose(x)
            k += 1
            small = M.branch_log(x[:9])
            th = _theta_of(T[0])
            cand = {b: M.se3_log(T, small=b) for b in (True, False)} if th > 1e-5 else None     # (below: the two agree to rounding)
            if cand and _abs(M.flat(cand[True][:3]), cand[False][:3]) > 1e4 * ULP * th:
                near = min(cand, key=lambda b: _abs(y[:3], cand[b][:3]))
                assert near == small, (name, x, near, small)
                taken[small] += 1
            if name == "float32 matrices":
                continue                                             # no exact logarithm of a matrix that is no rotation
            E = M.log_exact(T)
            nt = float(np.linalg.norm(x[9:]))
            b = RECORD[("log", name)][3] * _log_cond(x)
            tol_w = (th ** 3 / 6 if small else 0.0) + b * float(max(abs(v) for v in E[:3]))
            tol_v = (th ** 3 / 12 * (1 + th) * nt if small else 0.0) + b * float(max(abs(v) for v in E[3:]))
            assert _abs(y[:3], E[:3]) <= tol_w, (name, x, _abs(y[:3], E[:3]), tol_w)
            assert _abs(y[3:], E[3:]) <= tol_v, (name, x, _abs(y[3:], E[3:]), tol_v)
    assert taken[True] >= 20 and taken[False] >= 100, taken
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]


def test_log_of_exp_round_trips(oracle):
    """se3_log(se3_exp(u)) on the device: against the two formulas composed in 50 digits under the rule of exp and log (4 x the
    oracle's own round trip, at least 16 ulp, scaled by the logarithm's conditioning near pi), and against u itself within that
    plus the truncations: below theta = 4.5 mrad the logarithm's, below 1e-5 also the exponential's (|dR| <= theta^2 moves omega
    by as much, its first-order V moves upsilon by (theta / 2 + theta^2) |upsilon|, through a V^-1 that is I up to theta)"""
    groups = exp_inputs()
    cond = lambda x: max(1.0, 1.0 / (math.pi - float(np.linalg.norm(x[:3]))) ** 2)
    dev, X, worst = _against_oracle("log_exp", groups, lambda u: M.se3_log(M.se3_exp(M.vec(u))),
                                    lambda u: oracle.se3_log(oracle.se3_exp(u)), TWIST_BLOCKS, cond=cond)
    k = 0
    for name, G in groups.items():
        B = RECORD[("log_exp", name)][3]
        for x in G:
            y = dev[k]
            k += 1
            th, nu = float(np.linalg.norm(x[:3])), float(np.linalg.norm(x[3:]))
            small_exp, small_log = M.branch_exp(x), M.branch_log(M.se3_exp(M.vec(x))[0])
            tol_w = B * cond(x) * np.abs(x[:3]).max() + (th ** 3 / 6 if small_log else 0.0) + (th * th if small_exp else 0.0)
            tol_v = B * cond(x) * np.abs(x[3:]).max() + ((th ** 3 / 12) * (1 + th) * nu * (1 + th) if small_log else 0.0) \
                + ((0.5 * th + th * th) * nu * (1 + th) if small_exp else 0.0)
            dw, dv = np.abs(y[:3] - x[:3]).max(), np.abs(y[3:] - x[3:]).max()
            assert dw <= tol_w and dv <= tol_v, (name, x, dw, tol_w, dv, tol_v)
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]


# ---- mul -------------------------------------------------------------------------------------------------------------------------
def test_mul_same_formula(oracle):
    P = pairs()
    groups = {"random pairs": P[20:], "float32 rotations": P[:20]}
    _, _, worst = _against_oracle("mul", groups, lambda p: (lambda T: T[0] + T[1])(M.se3_mul(M.pose(p[:12]), M.pose(p[12:]))),
                                  lambda p: _p12(oracle.se3_mul(_T44(p[:12]), _T44(p[12:]))), POSE_BLOCKS)
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]


# ---- the straight-line functions -----------------------------------------------------------------------------------------------
def _straight(op, X, formula, operand=lambda x: np.abs(x).max(), scale=lambda x: 1.0, name="all"):
    dev = _device(op, X)
    worst = 0.0
    for x, y in zip(X, dev):
        ref = formula(x)
        bound = STRAIGHT * np.spacing(operand(x)) * scale(x)
        d = _abs(y, ref)
        worst = max(worst, d / bound)
        assert d <= bound, (op, name, x, d, bound)
    RECORD[(op, name)] = (len(X), None, worst, 1.0)
    print("%-12s %-40s n %3d  largest share of the 64-ulp bound %.3g" % (op, name, len(X), worst))
    return dev


def test_quat_of_and_normalize_rotation_every_branch_and_tie():
    seen = set()
    for name, G in rotations().items():
        b = [M.branch_quat(r) for r in G]
        seen |= set(b)
        if name.startswith("trace <= 0"):
            assert set(b) == {1 + int(name[13])}, (name, b)
        q = _straight("quat_of", G, lambda r: M.quat_of(M.vec(r)), operand=lambda r: 1.0, name=name)
        _straight("normalize", G, lambda r: M.normalize_rotation(M.vec(r)), operand=lambda r: 1.0, name=name)
        if name.startswith("half turns"):
            assert sorted(set(b)) == [1, 2, 3]
            for r, y, bi in zip(G, q, b):
                # w = 0 to the bit, so nothing flips the sign: the component the branch takes the root of is the positive one.  Another
                # branch would return the same quaternion up to its sign, and the sign shows which one it was.
                assert y[0] == 0.0 and y[bi] > 0.5, (r, y, bi)
    assert seen == {0, 1, 2, 3}


def test_to_mqt_and_from_mqt_on_both_sides_of_the_unit_sphere():
    P = poses(20240607, 60, f32=10)
    _straight("to_mqt", P, lambda p: M.to_mqt(M.pose(p)), operand=lambda p: 1.0)
    for name, G in mqt_inputs().items():
        outside = [M.branch_from_mqt(v) for v in G]
        if "+" in name:
            assert any(outside)
        w_of = lambda v: max(float(1 - (M.F(float(v[3])) ** 2 + M.F(float(v[4])) ** 2 + M.F(float(v[5])) ** 2)), ULP)
        dev = _straight("from_mqt", G, lambda v: (lambda T: T[0] + T[1])(M.from_mqt(M.vec(v))), operand=lambda v: 1.0,
                        scale=lambda v: 1.0 if M.branch_from_mqt(v) else max(1.0, 1.0 / math.sqrt(w_of(v))), name=name)
        for v, y, o in zip(G, dev, outside):
            assert np.array_equal(y[9:], v[:3])
            assert np.array_equal(y[:9], np.eye(3).reshape(-1)) == o, (name, v, y)        # the branch the device took
    assert any(M.branch_from_mqt(v) for v in mqt_inputs()["|q| = 1 and 1 + 1 ulp, one axis"][6:])
    assert not any(M.branch_from_mqt(v) for v in mqt_inputs()["|q| = 1 - 1 ulp, one axis"])


def test_adj():
    P = poses(20240608, 80, f32=10)
    dev = _straight("adj", P, lambda p: M.se3_adj(M.pose(p)))
    assert not dev.reshape(-1, 6, 6)[:, :3, 3:].any()


def test_mqt_jacobians_against_the_formula_and_central_differences():
    E = np.concatenate([poses(20240609, 60), np.c_[np.concatenate([g for n, g in rotations().items() if n.startswith("trace")]),
                                                    np.random.default_rng(5).normal(0, 2000.0, (72, 3))]])
    _straight("jac_right", E, lambda p: M.mqt_jac_right(M.pose(p)), name="formula")
    _straight("jac_right", E, lambda p: M.jac_right_fd(M.pose(p)), name="central differences")
    P = pairs()
    sign = np.array([float(M.wprod(M.pose(p[:12]), M.pose(p[12:]))) for p in P])
    assert (sign < -0.05).sum() >= 30 and (sign > 0.05).sum() >= 30, ((sign < 0).sum(), (sign > 0).sum())
    clear = np.abs(sign) > 1e-3                     # (a product that is zero to rounding has no sign to ask for)
    dev = _straight("jac_left_inv", P[clear], lambda p: M.mqt_jac_left_inv(M.pose(p[:12]), M.pose(p[12:])), name="formula")
    for p, y, s in zip(P[clear], dev, sign[clear]):
        # the branch the device took: the rotation block with the other sign is the other branch's
        other = M.mqt_jac_left_inv(M.pose(p[:12]), M.pose(p[12:]), negative=not s < 0)
        assert _abs(y, other) > 0.1, (p, s)
    orth = clear.copy()
    orth[:20] = False                               # float32 rotations: the formula assumes unit quaternions, the differences do not
    _straight("jac_left_inv", P[orth], lambda p: M.jac_left_inv_fd(M.pose(p[:12]), M.pose(p[12:])), name="central differences")


def write_record(path):
    """run on a machine with the device: every test above, then the figures as a table"""
    from oracle import oracle
    test_exp_same_formula_branch_and_exact_map(oracle)
    test_log_same_formula_branch_and_exact_map(oracle)
    test_log_of_exp_round_trips(oracle)
    test_mul_same_formula(oracle)
    test_quat_of_and_normalize_rotation_every_branch_and_tie()
    test_to_mqt_and_from_mqt_on_both_sides_of_the_unit_sphere()
    test_adj()
    test_mqt_jacobians_against_the_formula_and_central_differences()
    with open(path, "w") as f:
        f.write("| op | inputs | n | oracle to mpmath | device to mpmath | bound |\n|---|---|---|---|---|---|\n")
        for (op, name), (n, d_or, d_dev, bound) in RECORD.items():
            f.write("| %s | %s | %d | %s | %.2e | %.2e |\n" % (op, name.replace("|", "\\|"), n, "-" if d_or is None else "%.2e" % d_or, d_dev, bound))
    print("wrote", path, "(%d inputs)" % sum(v[0] for v in RECORD.values()))


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_record(sys.argv[1])
