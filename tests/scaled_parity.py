"""The distance between two normal-equation systems in their own scale (as tests/ba_cases.py: no tests, no fixtures).

The BA systems mix millimetres and radians: a rotation diagonal of 5e7 stands next to translation diagonals of 1 ... 18, and
`max |A - A_ref| <= tol * max |A_ref|` cannot tell most translation entries from zero.  Here every entry is divided by
d_i d_j with d = sqrt(|diag(A_ref)|) - the Jacobi scaling, in which the diagonal of A_ref is 1 and an off-diagonal entry is
the correlation of its two unknowns - so an entry between two translations weighs as much as one between two rotations.

The bound comes from the reference alone: with x the solution of A x = b and kappa the condition number of the scaled A,
an error dA of the scaled system moves the scaled x by at most kappa * |dA| relative (first order), so |dA| <= 1e-7 / kappa keeps a
step within 1e-7 = 1 % of the 1e-5 the suite asks of cost and pose updates (BASELINE.json north_star).  kappa is taken at
lambda = 0 for every lambda: damping only lowers it, and Levenberg-Marquardt may drive lambda down."""
import dataclasses

import numpy as np

STEP_SHARE = 1e-7        # 1 % of the north star's 1e-5
OLD_SE2, OLD_6DOF = 1e-11, 1e-10      # the bounds of the unscaled assertions (tests/test_ba_gpu.py; the 6-DoF models' files)


def jacobi(A_ref):
    """d = sqrt(|diag(A_ref)|), 1 where the diagonal is 0"""
    d = np.sqrt(np.abs(np.diag(np.asarray(A_ref))))
    return np.where(d == 0, 1.0, d)


def scaled_distance(A, A_ref):
    """max_ij |A - A_ref|_ij / (d_i d_j)"""
    d = jacobi(A_ref)
    return float((np.abs(np.asarray(A) - np.asarray(A_ref)) / np.outer(d, d)).max())


def scaled_rhs_distance(b, b_ref, A_ref):
    """max_i (|b - b_ref|_i / d_i) / max_i (|b_ref|_i / d_i)"""
    d = jacobi(A_ref)
    return float((np.abs(np.asarray(b) - np.asarray(b_ref)) / d).max() / (np.abs(np.asarray(b_ref)) / d).max())


def scaled_asymmetry(A, A_ref):
    """max_ij |A - A'|_ij / (d_i d_j): the symmetry check in the same scaling"""
    A = np.asarray(A)
    d = jacobi(A_ref)
    return float((np.abs(A - A.T) / np.outer(d, d)).max())


def kappa_scaled(A_ref):
    """condition number (2-norm) of A_ref / (d d')"""
    d = jacobi(A_ref)
    return float(np.linalg.cond(np.asarray(A_ref, np.float64) / np.outer(d, d)))


def bound(A_ref_lambda0):
    """the derived tolerance of scaled_distance and scaled_rhs_distance: STEP_SHARE / kappa_scaled of the reference's system at
    lambda = 0.  Computed from the reference, never from the implementation under test."""
    return STEP_SHARE / kappa_scaled(A_ref_lambda0)


def old_distance(A, A_ref):
    """max |A - A_ref| / max |A_ref|: the unscaled measure, for the record and for the statement of the gap"""
    return float(np.abs(np.asarray(A) - np.asarray(A_ref)).max() / np.abs(np.asarray(A_ref)).max())


def close(A, b, A_ref, b_ref, tol, what=None):
    """(scaled_distance, scaled_rhs_distance, scaled_asymmetry), each asserted <= tol"""
    dA, db, ds = scaled_distance(A, A_ref), scaled_rhs_distance(b, b_ref, A_ref), scaled_asymmetry(A, A_ref)
    print(f"scaled parity {what}: matrix {dA:.2e}, right-hand side {db:.2e}, asymmetry {ds:.2e}, bound {tol:.2e}")
    assert dA <= tol and db <= tol and ds <= tol, (what, dA, db, ds, tol)
    return dA, db, ds


def step_distance(x, x_ref, dof):
    """max over the component classes c (x, y, theta for dof = 3) of max |x - x_ref|_c / max |x_ref|_c: every class against its
    own maximum, as ba_cases.pose_update_close does, so that radians are not measured in millimetres"""
    x, x_ref = np.asarray(x, np.float64), np.asarray(x_ref, np.float64)
    return float(max(np.abs(x[c::dof] - x_ref[c::dof]).max() / np.abs(x_ref[c::dof]).max() for c in range(dof)))


# ---- the floor: the reference against itself with its edges in another order ------------------------------------------------
PERMS = (0, 1, 2, "reverse")      # three seeded permutations and the reversal


def permute_edges(g, how):
    """`g` with its projection edges (e_* arrays, length E) and its odometry edges (o_* arrays, length O) in another order:
    `how` = "reverse" or the seed of a permutation"""
    def order(n):
        return np.arange(n)[::-1] if how == "reverse" else np.random.default_rng(how).permutation(n)
    names = [f.name for f in dataclasses.fields(g)]
    new = {}
    for prefix, key in (("e_", "e_kf"), ("o_", "o_i")):
        if key not in names:
            continue
        p = order(len(getattr(g, key)))
        for n in names:
            if n.startswith(prefix) and getattr(g, n) is not None:
                new[n] = np.ascontiguousarray(np.asarray(getattr(g, n))[p])
    return dataclasses.replace(g, **new)


def reorder_floor(oracle_fn, g, perms=PERMS):
    """the largest scaled distance (matrix, right-hand side) of oracle_fn(g) -> (A, b) to itself over the edge orders `perms`:
    what a mere re-association of the sums costs.  For the record, not a bound."""
    A0, b0 = oracle_fn(g)
    out = [(scaled_distance(A, A0), scaled_rhs_distance(b, b0, A0)) for A, b in (oracle_fn(permute_edges(g, h)) for h in perms)]
    return max(a for a, _ in out), max(b for _, b in out)


# ---- mutations a good measure must see ---------------------------------------------------------------------------------------
# the translation unknowns inside a key frame's block: SE(2) (x, y, theta); SE3-expmap (omega, upsilon), g2o's order; the pose
# graph's VertexSE3 (t, vector part of q)
SE2, SE3, PG = (3, (0, 1)), (6, (3, 4, 5)), (6, (0, 1, 2))


def scale_translation_couplings(A, model, factor=1.001):
    """every translation-translation block between two DIFFERENT key frames times `factor`: 0.1 % in all position couplings"""
    dof, trans = model
    A = np.array(A, np.float64)
    idx = np.arange(A.shape[0])
    t = np.isin(idx % dof, trans)
    kf = idx // dof
    A[np.outer(t, t) & (kf[:, None] != kf[None, :])] *= factor
    return A


def zero_smallest(A, share=0.25):
    """the smallest `share` of the non-zero entries (by magnitude) set to zero"""
    A = np.array(A, np.float64)
    nz = np.abs(A[A != 0])
    cut = np.sort(nz)[int(share * nz.size)]
    A[np.abs(A) < cut] = 0.0
    return A


# ---- the SE(2) reduced system from the compiled reference's own edges, in any precision -----------------------------------------
def _inv3(M):
    """3 x 3 inverse by cofactors, in M's dtype (np.linalg.inv has no longdouble)"""
    a, b, c, d, e, f, g, h, i = M.reshape(9)
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                    [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]], M.dtype)
    return adj / (a * adj[0, 0] + b * adj[1, 0] + c * adj[2, 0])


def reference_edges(g):
    """residual and Jacobians of every edge of an SE(2) window from the COMPILED REFERENCE (oracle/_ref: g2o::EdgeSE2XYZ and
    PreEdgeSE2 as the reference writes them) -> (projection edges [(e, Jp, Jl)], odometry edges [(e, Ji, Jj)]), in double"""
    from oracle import ref
    proj = [ref.edge_se2xyz(g, g.poses[int(g.e_kf[k])], g.lms[int(g.e_lm[k])], g.e_uv[k]) for k in range(g.E)]
    odo = [ref.edge_pre_se2(g.poses[int(g.o_i[k])], g.poses[int(g.o_j[k])], g.o_meas[k]) for k in range(g.O)]
    return proj, odo


def se2_system_from_reference_edges(g, lam, dtype=np.float64, edges=None):
    """The Schur-reduced pose system (S, b) of an SE(2) window assembled in numpy, in `dtype`, from the compiled reference's
    residuals and Jacobians: robust weights and constructQuadraticForm as g2o defines them (H += J' rho' Omega J,
    b -= J' rho' Omega e), S = Hpp + lam I - sum_l B_l (Hll_l + lam I)^-1 B_l', the identity on fixed key frames.  With
    dtype = np.longdouble every sum, product and inverse after the per-edge values runs in extended precision: the adjudicator
    between two double-precision assemblies that associate differently."""
    T = dtype
    proj, odo = reference_edges(g) if edges is None else edges
    P, L = g.P, g.L
    n = 3 * P
    lam = T(lam)
    I3 = np.eye(3, dtype=T)
    Hpp = np.zeros((n, n), T); bp = np.zeros(n, T); Hll = np.zeros((L, 3, 3), T); bl = np.zeros((L, 3), T)
    by_lm = {}
    for k, (e, Jp, Jl) in enumerate(proj):
        kf, lm = int(g.e_kf[k]), int(g.e_lm[k])
        e, Jp, Jl = e.astype(T), Jp.astype(T), Jl.astype(T)
        w = np.asarray(g.e_info[k], T)
        Om = np.array([[w[0], w[1]], [w[1], w[2]]], T)
        e2 = e @ Om @ e
        r1 = T(1) if e2 <= T(g.huber) ** 2 else T(g.huber) / np.sqrt(e2)
        Hll[lm] += Jl.T @ (r1 * Om) @ Jl
        bl[lm] -= Jl.T @ (r1 * Om) @ e
        if not g.fixed[kf]:
            s = slice(3 * kf, 3 * kf + 3)
            Hpp[s, s] += Jp.T @ (r1 * Om) @ Jp
            bp[s] -= Jp.T @ (r1 * Om) @ e
            by_lm.setdefault(lm, []).append((kf, Jp.T @ (r1 * Om) @ Jl))
    for k, (e, A, B) in enumerate(odo):
        i, j = int(g.o_i[k]), int(g.o_j[k])
        e, A, B = e.astype(T), A.astype(T), B.astype(T)
        W = np.asarray(g.o_info[k], T).reshape(3, 3)
        for a, Ja in ((i, A), (j, B)):
            if g.fixed[a]:
                continue
            bp[3 * a:3 * a + 3] -= Ja.T @ W @ e
            for b, Jb in ((i, A), (j, B)):
                if not g.fixed[b]:
                    Hpp[3 * a:3 * a + 3, 3 * b:3 * b + 3] += Ja.T @ W @ Jb
    S, bs = Hpp, bp
    for p in range(P):
        s = slice(3 * p, 3 * p + 3)
        if g.fixed[p]:
            S[s, s] = I3
        else:
            S[s, s] += lam * I3
    for lm, obs in by_lm.items():
        Dinv = _inv3(Hll[lm] + lam * I3)
        for a, Ba in obs:
            BaD = Ba @ Dinv
            bs[3 * a:3 * a + 3] -= BaD @ bl[lm]
            for b, Bb in obs:
                S[3 * a:3 * a + 3, 3 * b:3 * b + 3] -= BaD @ Bb.T
    return S, bs
