"""Checks that do NOT come from the oracle's restatement ("pin the oracle").

Everything here is written against the *definitions* (the generator's projection model, the textbook bilinear /
Gaussian formulas, scipy's trust-region least squares), never against oracle/*.cpp or the HIP kernels, so that a
convention error shared by the restatement and the kernels cannot hide:

* `BAProblemNumpy`   the robust cost  sum_e rho_huber(r_e' Omega_e r_e) + sum_o r_o' Omega_o r_o  of a synth.BAGraph as a
                     plain numpy residual vector (projection = synth._project, the function that GENERATED the
                     measurements), suitable for scipy.optimize.least_squares with a finite-difference Jacobian.
* `bilinear_half_pixel`, `gaussian_float`   float references of cv::resize(INTER_LINEAR) and cv::GaussianBlur(7x7, 2).
"""
from __future__ import annotations

import numpy as np

from se2lam_amd import synth


class BAProblemNumpy:
    """g2o's cost for Map::loadLocalGraph's graph (src/Map.cpp:891-1053), from the definitions:
    EdgeSE2XYZ error = project(pose, landmark) - uv with RobustKernelHuber(delta) on e' Omega e
    (rho = s if s <= delta^2 else 2 delta sqrt(s) - delta^2), PreEdgeSE2 error = (R_i'(t_j - t_i) - z_xy, th_j - th_i - z_th)
    without a robust kernel.  fun(x) returns a vector f with ||f||^2 = that cost: per observation the whitened residual
    scaled by sqrt(rho(s)/s)."""

    def __init__(self, g):
        self.g = g
        self.Rcb = g.Rbc.T
        self.tcb = -self.Rcb @ g.tbc
        self.free = np.nonzero(g.fixed == 0)[0]
        self.npz = 3 * self.free.size
        W = np.zeros((g.E, 2, 2))
        W[:, 0, 0] = g.e_info[:, 0]
        W[:, 0, 1] = W[:, 1, 0] = g.e_info[:, 1]
        W[:, 1, 1] = g.e_info[:, 2]
        self.U = np.linalg.cholesky(W).transpose(0, 2, 1)                       # Omega = U' U
        self.Uo = np.linalg.cholesky(g.o_info.reshape(g.O, 3, 3)).transpose(0, 2, 1) if g.O else np.zeros((0, 3, 3))

    def pack(self, poses, lms):
        return np.concatenate([np.asarray(poses)[self.free].reshape(-1), np.asarray(lms).reshape(-1)])

    def unpack(self, x):
        poses = self.g.poses.copy()
        poses[self.free] = x[:self.npz].reshape(-1, 3)
        return poses, x[self.npz:].reshape(self.g.L, 3)

    def fun(self, x):
        g = self.g
        poses, lms = self.unpack(x)
        u, v, _, _ = synth._project(poses, lms, g.e_kf, g.e_lm, self.Rcb, self.tcb, g.fx, g.cx, g.cy)
        r = np.stack([u - g.e_uv[:, 0], v - g.e_uv[:, 1]], 1)
        wr = np.einsum("eij,ej->ei", self.U, r)
        s = (wr * wr).sum(1)
        d2 = g.huber ** 2
        rho = np.where(s <= d2, s, 2 * np.sqrt(np.maximum(s, 1e-300)) * g.huber - d2)
        k = np.sqrt(rho / np.maximum(s, 1e-300))
        pi, pj = poses[g.o_i], poses[g.o_j]
        c, sn = np.cos(pi[:, 2]), np.sin(pi[:, 2])
        dx, dy = pj[:, 0] - pi[:, 0], pj[:, 1] - pi[:, 1]
        e = np.stack([c * dx + sn * dy - g.o_meas[:, 0], -sn * dx + c * dy - g.o_meas[:, 1],
                      pj[:, 2] - pi[:, 2] - g.o_meas[:, 2]], 1)          # no angle wrap: EdgeSE2XYZ.h:80
        return np.concatenate([(wr * k[:, None]).reshape(-1), np.einsum("eij,ej->ei", self.Uo, e).reshape(-1)])

    def cost(self, poses, lms):
        f = self.fun(self.pack(poses, lms))
        return float(f @ f)

    def sparsity(self):
        from scipy.sparse import coo_matrix
        g = self.g
        slot = -np.ones(g.P, int)
        slot[self.free] = np.arange(self.free.size)
        rows, cols = [], []
        for k3 in range(3):
            for rr in range(2):
                a = slot[g.e_kf]
                m = a >= 0
                rows.append((2 * np.arange(g.E) + rr)[m]); cols.append(3 * a[m] + k3)
                rows.append(2 * np.arange(g.E) + rr); cols.append(self.npz + 3 * g.e_lm + k3)
            for rr in range(3):
                for q in (g.o_i, g.o_j):
                    a = slot[q]
                    m = a >= 0
                    rows.append((2 * g.E + 3 * np.arange(g.O) + rr)[m]); cols.append(3 * a[m] + k3)
        rows = np.concatenate(rows); cols = np.concatenate(cols)
        return coo_matrix((np.ones(rows.size, np.int8), (rows, cols)),
                          shape=(2 * g.E + 3 * g.O, self.npz + 3 * g.L)).tocsr()

    def solve(self, x0, max_nfev=200):
        """scipy's trust-region reflective least squares on fun, finite-difference Jacobian (exact SVD steps for small
        graphs, LSMR + sparsity pattern otherwise)."""
        from scipy.optimize import least_squares
        dense = x0.size <= 600
        return least_squares(self.fun, x0, jac="3-point", jac_sparsity=None if dense else self.sparsity(), method="trf",
                             x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-13, max_nfev=max_nfev,
                             tr_solver="exact" if dense else "lsmr")


def bilinear_half_pixel(src: np.ndarray, w: int, h: int) -> np.ndarray:
    """Float bilinear resize with the half-pixel mapping  sx = (dx + 0.5) * (sw / w) - 0.5  and edge clamping - the
    definition of cv::resize(..., INTER_LINEAR) (and of torch interpolate(align_corners=False)) - in float64."""
    sh, sw = src.shape
    s = src.astype(np.float64)
    fx = (np.arange(w) + 0.5) * (sw / w) - 0.5
    fy = (np.arange(h) + 0.5) * (sh / h) - 0.5
    x0 = np.floor(fx).astype(int); y0 = np.floor(fy).astype(int)
    ax = fx - x0; ay = fy - y0
    x0c, x1c = np.clip(x0, 0, sw - 1), np.clip(x0 + 1, 0, sw - 1)
    y0c, y1c = np.clip(y0, 0, sh - 1), np.clip(y0 + 1, 0, sh - 1)
    top = s[y0c][:, x0c] * (1 - ax) + s[y0c][:, x1c] * ax
    bot = s[y1c][:, x0c] * (1 - ax) + s[y1c][:, x1c] * ax
    return top * (1 - ay)[:, None] + bot * ay[:, None]


def gaussian_float(src: np.ndarray, ksize: int = 7, sigma: float = 2.0) -> np.ndarray:
    """Float separable Gaussian (cv::getGaussianKernel: exp(-(i-c)^2 / 2 sigma^2), normalised) with BORDER_REFLECT_101."""
    c = (ksize - 1) / 2
    k = np.exp(-((np.arange(ksize) - c) ** 2) / (2 * sigma * sigma))
    k /= k.sum()
    r = ksize // 2
    p = np.pad(src.astype(np.float64), r, mode="reflect")          # numpy 'reflect' == BORDER_REFLECT_101
    tmp = sum(k[i] * p[:, i:i + src.shape[1]] for i in range(ksize))
    return sum(k[i] * tmp[i:i + src.shape[0], :] for i in range(ksize))


class BA3ProblemNumpy:
    """The SE3-expmap local BA cost (Map.cpp:414-566) from the definitions, with numpy / scipy.spatial only:
    sum_e rho_huber(w_e |uv - pi(T X)|^2) + sum_a |log(M_a T_a^-1)|^2_Omega_a + sum_o |log(T_j^-1 C T_i)|^2_Omega_o."""

    def __init__(self, g, log=None):
        self.g = g
        self.log = synth.se3_log_np if log is None else log      # the exact logarithm, or g2o's (se3_log_g2o below)

    def cost(self, poses, lms):
        g = self.g
        T = np.asarray(poses)
        Xc = np.einsum("eij,ej->ei", T[g.e_kf][:, :3, :3], np.asarray(lms)[g.e_lm]) + T[g.e_kf][:, :3, 3]
        u = g.fx * Xc[:, 0] / Xc[:, 2] + g.cx
        v = g.fx * Xc[:, 1] / Xc[:, 2] + g.cy
        s = g.e_w * ((g.e_uv[:, 0] - u) ** 2 + (g.e_uv[:, 1] - v) ** 2)
        d2 = g.huber ** 2
        self.edge_chi2 = s
        chi = np.where(s <= d2, s, 2 * np.sqrt(s) * g.huber - d2).sum()
        for a in range(g.P):
            if g.has_prior[a]:
                e = self.log(g.prior_meas[a] @ np.linalg.inv(T[a]))
                chi += e @ g.prior_info[a] @ e
        for k in range(g.O):
            e = self.log(np.linalg.inv(T[g.o_j[k]]) @ g.o_meas[k] @ T[g.o_i[k]])
            chi += e @ g.o_info[k] @ e
        return float(chi)


def se3_log_g2o(T):
    """SE3Quat::log as g2o defines it, (omega, upsilon): with d = (tr R - 1) / 2 and (R - R')^v the vector of the antisymmetric
    part, omega = (R - R')^v / 2 and V^-1 = I - Omega / 2 + Omega^2 / 12 when d > 0.99999 (below 4.5 mrad: first order), else
    omega = theta / (2 sqrt(1 - d^2)) (R - R')^v and V^-1 = I - Omega / 2 + (1 - theta / (2 tan(theta / 2))) / theta^2 Omega^2"""
    R, t = T[:3, :3], T[:3, 3]
    d = 0.5 * (np.trace(R) - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if d > 0.99999:
        w, c = 0.5 * dR, 1.0 / 12.0
    else:
        th = np.arccos(d)
        w, c = th / (2 * np.sqrt(1 - d * d)) * dR, (1 - th / (2 * np.tan(th / 2))) / th ** 2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    return np.concatenate([w, (np.eye(3) - 0.5 * K + c * K @ K) @ t])


def ba3_full_normal_equations(g, lam, log=se3_log_g2o):
    """The full (6P + 3L) Levenberg-Marquardt normal equations H dx = b of a synth.BA3Graph at its own estimate, from the definitions
    of the three edge types (g2o's types_six_dof_expmap and the reference's EdgeSE3ExpmapPrior), every vertex updated as
    exp(d) * T with d = (omega, upsilon) or X + d:
      EdgeProjectXYZ2UV   e = uv - pi(T X), p = T X: de/dX = -dpi/dp R, de/dd = -dpi/dp [-[p]x  I]; information w I, Huber weight
                          rho' = 1 if w |e|^2 <= delta^2 else delta / sqrt(w |e|^2), on these edges only
      EdgeSE3ExpmapPrior  e = log(M T^-1), J = -I (the reference's linearizeOplus; its adjoint forms are commented out there)
      EdgeSE3Expmap       e = log(T_j^-1 C T_i), J_i = adj(T_j^-1 C), J_j = -adj(T_i^-1 C^-1)
    H = sum J' rho' W J + lam I, b = -sum J' rho' W e.  Fixed poses keep their rows here: the caller deletes them.
    -> (H, b), unknowns ordered poses then landmarks."""
    P, L = g.P, g.L
    N = 6 * P + 3 * L
    H, b = np.zeros((N, N)), np.zeros(N)

    def add(cols, Js, W, e):
        idx = np.concatenate(cols)
        J = np.concatenate(Js, axis=1)
        H[np.ix_(idx, idx)] += J.T @ W @ J
        b[idx] -= J.T @ W @ e

    T = np.asarray(g.poses)
    for k in range(g.E):
        a, l = int(g.e_kf[k]), int(g.e_lm[k])
        R = T[a][:3, :3]
        p = R @ g.lms[l] + T[a][:3, 3]
        x, y, z = p
        e = g.e_uv[k] - np.array([g.fx * x / z + g.cx, g.fx * y / z + g.cy])
        dpi = g.fx / z * np.array([[1, 0, -x / z], [0, 1, -y / z]])
        px = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0.0]])
        s = g.e_w[k] * (e @ e)
        rho1 = 1.0 if s <= g.huber ** 2 else g.huber / np.sqrt(s)
        add([np.arange(6 * a, 6 * a + 6), np.arange(6 * P + 3 * l, 6 * P + 3 * l + 3)],
            [-dpi @ np.concatenate([-px, np.eye(3)], axis=1), -dpi @ R], rho1 * g.e_w[k] * np.eye(2), e)
    for a in range(P):
        if g.has_prior[a]:
            add([np.arange(6 * a, 6 * a + 6)], [-np.eye(6)], g.prior_info[a], log(g.prior_meas[a] @ np.linalg.inv(T[a])))
    for k in range(g.O):
        i, j = int(g.o_i[k]), int(g.o_j[k])
        C = g.o_meas[k]
        e = log(np.linalg.inv(T[j]) @ C @ T[i])
        Ji = synth.se3_adj_np(np.linalg.inv(T[j]) @ C)
        Jj = -synth.se3_adj_np(np.linalg.inv(T[i]) @ np.linalg.inv(C))
        add([np.arange(6 * i, 6 * i + 6), np.arange(6 * j, 6 * j + 6)], [Ji, Jj], g.o_info[k], e)
    H += lam * np.eye(N)
    return H, b


# ------------------------------------------------------------------------------------------------------------------
# Tracking / mapping thread kernels (csrc/triangulate.hip, ransac.hip, pose_ba.hip, sparsify.hip): references written from
# the definitions with numpy / scipy only.  Each check_* function takes the inputs and ONE implementation's outputs (the CPU
# restatement's or the HIP path's - the same checker serves both) and raises AssertionError; it returns the measured figures.
# ------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24          # unit round-off of float
U64 = 2.0 ** -53
MIN_COS = (0.9998, 0.9994, 0.9986, 0.9976)   # cvu::checkParallax, minDegree 1..4 (as floats in the kernel)

# Constant of the singular-vector term of the triangulation tolerance, see triangulation_reference.  LAPACK's dgesdd and a
# one-sided Jacobi SVD are both backward stable: each returns the exact singular vectors of A + E with |E| <= p(4) * 2^-52 * s1
# for a modest polynomial p of the dimension.  The two vectors then differ by at most (|E_lapack| + |E_jacobi|) / gap.  C = 8
# allows p(4) = 4 (the dimension) on each side; it was fixed from this argument before any HIP output was looked at, and the
# restatement needs less than 1 % of it on every scene of the suite (profiles/track_independent.md).
TRI_C = 8.0


def triangulation_reference(kps_ref, kps_cur, match_idx, P_ref, P_cur):
    """cvu::triangulate (cvutil.cpp:46-59) from its definition: the 4x4 system built in float exactly as the cv::Mat
    arithmetic does (those float rows ARE the input), widened, numpy's (LAPACK's) SVD, the last right singular vector
    dehomogenised in FP64.  -> X (n,3) f64 (NaN rows where unmatched), tol (n,3) absolute per coordinate, sv (n,4).
    Tolerance, derived: the implementation rounds v0..v3 to float and divides in float - three roundings per coordinate,
    3 * 2^-24 relative to the coordinate; and its unit singular vector may differ from LAPACK's by eta = TRI_C * 2^-52 *
    s1 / (s3 - s4) (perturbation of a simple singular vector, gap to the nearest other singular value), which moves
    X_c = v_c / v_3 by at most eta * (1 + |X_c|) / |v_3| = eta * (1 + |X_c|) * |(X, 1)|."""
    n = len(kps_ref)
    m = np.asarray(match_idx)
    sel = np.flatnonzero(m >= 0)
    X = np.full((n, 3), np.nan); tol = np.full((n, 3), np.nan); sv = np.full((n, 4), np.nan)
    if sel.size == 0:
        return X, tol, sv
    P1 = np.asarray(P_ref, np.float32).reshape(3, 4); P2 = np.asarray(P_cur, np.float32).reshape(3, 4)
    x1 = kps_ref["x"][sel].astype(np.float32)[:, None]; y1 = kps_ref["y"][sel].astype(np.float32)[:, None]
    x2 = kps_cur["x"][m[sel]].astype(np.float32)[:, None]; y2 = kps_cur["y"][m[sel]].astype(np.float32)[:, None]
    A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]], 1)
    assert A.dtype == np.float32
    _, s, Vt = np.linalg.svd(A.astype(np.float64))
    v = Vt[:, 3, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        Xs = v[:, :3] / v[:, 3:]
        eta = TRI_C * 2.0 ** -52 * s[:, 0] / (s[:, 2] - s[:, 3])
        t = 3 * U32 * np.abs(Xs) + eta[:, None] * (1 + np.abs(Xs)) * np.sqrt(1 + (Xs * Xs).sum(1))[:, None]
    X[sel], tol[sel], sv[sel] = Xs, t, s
    return X, tol, sv


def check_triangulation(inputs, outputs, degenerate=False):
    """inputs = (kps_ref, kps_cur, match_idx, has_obs, P_ref, P_cur, Ocam, lower, upper, min_degree); outputs = (pos, good,
    match_out, n_good, n_tracked_old) of Track::doTriangulate.  Positions against triangulation_reference within its tolerance;
    the depth gate, the match_idx update, the parallax flag and both counters recomputed from the FP64 positions.  A point
    whose FP64 depth (parallax cosine) lies within the tolerance of a threshold may fall either way; at most 1 % of the matched
    points of a scene may be such points.  degenerate: the null space is not a line (P_cur == P_ref) - only "finite or dropped,
    never a NaN kept" is asserted.  -> dict(worst share of the tolerance used, borderline share)"""
    kps_ref, kps_cur, match_idx, has_obs, P_ref, P_cur, Ocam, lower, upper, min_degree = inputs
    pos, good, m_out, n_good, n_old = outputs
    n = len(kps_ref)
    m_in = np.asarray(match_idx, np.int32)
    pos = np.asarray(pos); good = np.asarray(good).astype(bool); m_out = np.asarray(m_out)
    assert pos.shape == (n, 3) and good.shape == (n,) and m_out.shape == (n,) and pos.dtype == np.float32
    obs = np.zeros(n, bool) if has_obs is None else np.asarray(has_obs).astype(bool)
    matched = m_in >= 0
    todo = matched & ~obs
    # the counters come from device atomics: they must equal what the arrays say, always
    assert n_good == int(good.sum()), (n_good, int(good.sum()))
    assert n_old == int((matched & obs).sum()), (n_old, int((matched & obs).sum()))
    # features that are not triangulated: untouched
    assert np.array_equal(m_out[~todo], m_in[~todo]) and not pos[~todo].any() and not good[~todo].any()
    kept = todo & (m_out >= 0)
    assert np.array_equal(m_out[kept], m_in[kept]) and (m_out[todo & ~kept] == -1).all()
    assert not pos[todo & ~kept].any() and not good[todo & ~kept].any()
    assert np.isfinite(pos).all()                                   # never a NaN kept, whatever the geometry
    assert (pos[kept, 2] >= np.float32(lower)).all() and (pos[kept, 2] <= np.float32(upper)).all()
    if degenerate or not todo.any():
        return dict(used=0.0, borderline=0.0)
    X, tol, _ = triangulation_reference(kps_ref, kps_cur, m_in, P_ref, P_cur)
    assert np.isfinite(X[todo]).all() and np.isfinite(tol[todo]).all()
    Z, tz = X[:, 2], tol[:, 2]
    lo, hi = float(np.float32(lower)), float(np.float32(upper))
    near_gate = todo & ((np.abs(Z - lo) <= tz) | (np.abs(Z - hi) <= tz))
    inside = (Z >= lo) & (Z <= hi)
    clear = todo & ~near_gate
    assert np.array_equal(kept[clear], inside[clear]), "depth gate differs from the FP64 depth outside the tolerance"
    used = np.abs(pos[kept].astype(np.float64) - X[kept]) / tol[kept]
    worst = float(used.max()) if used.size else 0.0
    assert worst <= 1.0, "position off by %.3g of the derived tolerance" % worst
    # cvu::checkParallax(o1 = 0, o2 = Ocam, pt3): cos = |p . (p - O)| / (|p| |p - O|) < minCos (a float constant).  Tolerance of
    # the cosine: d cos <= d angle <= |dp| / |p| + |dp| / |p - O| from the position tolerance, plus the float evaluation: one
    # rounding in each p - O, one per product, two sums, |dot| <= |p||q| and cos ~ 1: 4 * 2^-24 / cos; one for p - O inside the
    # norms; one for the final cast: 6 * 2^-24, taken as 8.
    O = np.asarray(Ocam, np.float32).astype(np.float64)
    q = X - O
    npn, nq = np.linalg.norm(X, axis=1), np.linalg.norm(q, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cosp = np.abs((X * q).sum(1)) / (npn * nq)
        tcos = 8 * U32 + np.linalg.norm(tol, axis=1) * (1 / npn + 1 / nq)
    mc = float(np.float32(MIN_COS[min_degree - 1]))
    near_cos = kept & (np.abs(cosp - mc) <= tcos)
    sure = kept & ~near_cos & ~near_gate
    assert np.array_equal(good[sure], cosp[sure] < mc), "parallax flag differs from the FP64 cosine outside the tolerance"
    share = float((near_gate | near_cos).sum()) / float(matched.sum())
    assert share <= 0.01, "%.2f %% of the matched points lie within the tolerance of a threshold" % (100 * share)
    return dict(used=worst, borderline=share)


# ---------------------------------------------------------------------------------------------------------- sparsifier
def _min_of(T):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(T[:3, :3]).as_quat()
    if q[3] < 0:
        q = -q
    return np.r_[T[:3, 3], q[:3]]


def _from_min(v):
    from scipy.spatial.transform import Rotation
    w2 = 1 - v[3:] @ v[3:]
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat([v[3], v[4], v[5], np.sqrt(max(w2, 0.0))]).as_matrix()
    T[:3, 3] = v[:3]
    return T


def sparsify_numpy_model(kf, mp, m_kf, m_mp, m_info):
    """Sparsifier::DoMarginalizeSE3XYZ from its definition: central-difference Jacobians of the minimal parametrisation with
    scipy's quaternions, dense Schur complement, numpy's inverse and eigh -> (z, information, marginal Hessian)"""
    N = len(mp)
    H = np.zeros((12 + 3 * N, 12 + 3 * N))
    h = 1e-6
    for k, m, W in zip(m_kf, m_mp, m_info):
        if k not in (0, 1):
            continue                                   # sparsifier.cpp:117-119
        v = _min_of(kf[k])
        f = lambda vv, pp: (np.linalg.inv(_from_min(vv)) @ np.r_[pp, 1.0])[:3]
        J = np.zeros((3, 9))
        for i in range(6):
            d = np.zeros(6); d[i] = h
            J[:, i] = (f(v + d, mp[m]) - f(v - d, mp[m])) / (2 * h)
        for i in range(3):
            d = np.zeros(3); d[i] = h
            J[:, 6 + i] = (f(v, mp[m] + d) - f(v, mp[m] - d)) / (2 * h)
        idx = np.r_[6 * k + np.arange(6), 12 + 3 * m + np.arange(3)]
        H[np.ix_(idx, idx)] += J.T @ W @ J
    H[:12, :12] += 1e-6 * np.eye(12)
    seen = np.flatnonzero(np.abs(H[12:, 12:]).reshape(N, 3, -1).sum((1, 2)) > 0) if N else np.zeros(0, int)
    pts = (12 + 3 * seen[:, None] + np.arange(3)).reshape(-1)      # points without a measurement drop out
    Hm = H[:12, :12] - (H[:12, pts] @ np.linalg.solve(H[np.ix_(pts, pts)], H[pts, :12]) if pts.size else 0.0)
    z = lambda a, b: _min_of(np.linalg.inv(_from_min(a)) @ _from_min(b))
    v1, v2 = _min_of(kf[0]), _min_of(kf[1])
    J = np.zeros((6, 12))
    for i in range(6):
        d = np.zeros(6); d[i] = h
        J[:, i] = (z(v1 + d, v2) - z(v1 - d, v2)) / (2 * h)
        J[:, 6 + i] = (z(v1, v2 + d) - z(v1, v2 - d)) / (2 * h)
    I = np.linalg.inv(J @ np.linalg.inv(Hm) @ J.T)
    I = 0.5 * (I + I.T)
    lam, U = np.linalg.eigh(I)
    lam = np.where(lam < 0, 1e-6, np.clip(lam, 1e-6, 1e4))
    return np.linalg.inv(kf[0]) @ kf[1], (U * lam) @ U.T, Hm


def check_sparsify(pair, z, info, model=None, spectrum=True):
    """One implementation's (z, information) of a key-frame pair against the numpy model: z = KF0^-1 KF1 to 1e-9, exact
    symmetry, the spectrum inside the clamp [1e-6, 1e4]; and with spectrum=True (pairs with enough points for the model to be
    well determined) the rotation eigenvalues at the 1e4 clamp and the translation ones within a factor 2 of the model's.
    (The step from the marginal Hessian to the information is ill-conditioned by construction - six gauge freedoms held by
    a 1e-6 regulariser - so forward against central differences move the small eigenvalues by tens of per cent.)"""
    kf = pair[0]
    z = np.asarray(z); info = np.asarray(info)
    assert np.isfinite(z).all() and np.isfinite(info).all()
    assert np.allclose(z, np.linalg.inv(kf[0]) @ kf[1], rtol=0, atol=1e-9)
    assert np.abs(info - info.T).max() == 0
    lam = np.linalg.eigvalsh(info)
    # (eigvalsh and the implementation's own V diag(lam) V' are each exact for a matrix 2^-52 |info| p(6) away, so an eigenvalue
    # sitting AT the 1e-6 floor of a matrix of norm 1e4 is only known to 64 * 2^-52 * 1e4 = 1.4e-10 absolute)
    assert lam.min() >= 1e-6 * (1 - 1e-9) - 64 * 2.0 ** -52 * lam.max() and lam.max() <= 1e4 * (1 + 1e-9)
    if not spectrum:
        return
    zn, infon, _ = sparsify_numpy_model(*pair) if model is None else model
    assert np.allclose(z, zn, rtol=0, atol=1e-9)
    ln = np.sort(np.linalg.eigvalsh(infon))
    lo = np.sort(lam)
    assert np.allclose(lo[3:], 1e4, rtol=1e-6) and np.allclose(ln[3:], 1e4, rtol=1e-6)
    assert np.all(lo[1:3] > 0.5 * ln[1:3]) and np.all(lo[1:3] < 2.0 * ln[1:3]) and 1e-6 <= lo[0] < lo[1]


def check_sparsify_equals(z, info, z_ref, info_ref):
    """an implementation's output against the restatement's FOR THE SAME MEASUREMENT ORDER: the suite's tolerances.  The bound
    is 1e-5 of the LARGEST entry - 0.1 absolute wherever a rotation eigenvalue sits at the 1e4 clamp - so the relative
    information distance is printed beside it (asserted only where the reference is not noise in it: check_sparsify_relative)"""
    assert np.allclose(z, z_ref, atol=1e-12)
    try:
        d = info_distance(info, info_ref)
    except np.linalg.LinAlgError:      # (a reference that is not positive definite to working precision: nothing to print)
        d = float("nan")
    print("sparsify: |info - ref| / max %.2e, relative information distance %.2e" % (np.abs(info - info_ref).max() / np.abs(info_ref).max(), d))
    assert np.abs(info - info_ref).max() <= 1e-5 * np.abs(info_ref).max(), np.abs(info - info_ref).max() / np.abs(info_ref).max()


def info_distance(info, info_ref):
    """max |w - 1| over the generalised eigenvalues w of (info, info_ref): the largest relative difference of the information the
    two matrices hold about any direction - millimetre and radian directions weigh the same, which max |info - ref| / max |ref|
    does not do (there the translation block may be 100 % off under a rotation block at the 1e4 clamp)"""
    import scipy.linalg
    return float(np.abs(scipy.linalg.eigh(np.asarray(info, np.float64), np.asarray(info_ref, np.float64), eigvals_only=True) - 1.0).max())


def sparsify_ulp_floor(sparsify, pair, draws=4, seed=0):
    """The reference's own noise in info_distance: the largest distance of sparsify(pair)'s information to that of `draws` copies
    of the pair in which every entry of m_info (kept symmetric) and of mp is moved by one ulp, up or down at random."""
    kf, mp, m_kf, m_mp, m_info = pair
    info0 = sparsify(*pair)[1]
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(3, 1)

    def ulp(a):
        a = np.asarray(a, np.float64)
        return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))
    out = []
    for _ in range(draws):
        mi = ulp(m_info)
        mi[:, iu[1], iu[0]] = mi[:, iu[0], iu[1]]
        out.append(info_distance(sparsify(kf, ulp(mp), m_kf, m_mp, mi)[1], info0))
    return max(out)


FLOOR_MARGIN = 64      # four draws undersample the floor


def check_sparsify_relative(z, info, z_ref, info_ref, floor):
    """an implementation against the restatement on a pair where the restatement is well determined: the information within
    FLOOR_MARGIN x the restatement's own one-ulp floor in the relative measure, and a rotation eigenvalue (the three largest)
    strictly inside the clamp (1e-6, 1e4) - the regime these pairs are there for"""
    assert np.allclose(z, z_ref, atol=1e-12)
    assert np.abs(info - info.T).max() == 0
    d = info_distance(info, info_ref)
    rot = np.sort(np.linalg.eigvalsh(info_ref))[3:]
    print("sparsify: relative information distance %.2e, one-ulp floor of the reference %.2e (bound %d x), rotation eigenvalues %s"
          % (d, floor, FLOOR_MARGIN, ["%.4g" % x for x in rot]))
    assert ((rot > 1e-6 * (1 + 1e-6)) & (rot < 1e4 * (1 - 1e-6))).any(), rot
    assert d <= FLOOR_MARGIN * floor, (d, floor)
    return d


# ------------------------------------------------------------------------------------------------------- pose-only BA
def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def se3_log_scipy(T):
    """log of a rigid transform in g2o's order (rotation vector, then V^-1 t), the rotation vector from scipy"""
    from scipy.spatial.transform import Rotation
    w = Rotation.from_matrix(T[:3, :3]).as_rotvec()
    th = np.linalg.norm(w)
    K = _hat(w)
    Vi = np.eye(3) - 0.5 * K + ((1 / 12.0) if th < 1e-6 else (1 - th / (2 * np.tan(th / 2))) / th ** 2) * K @ K
    return np.concatenate([w, Vi @ T[:3, 3]])


def se3_exp_scipy(d):
    from scipy.spatial.transform import Rotation
    w, v = np.asarray(d[:3], float), np.asarray(d[3:], float)
    th = np.linalg.norm(w)
    K = _hat(w)
    if th < 1e-6:
        V = np.eye(3) + 0.5 * K + K @ K / 6.0
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(w).as_matrix()
    T[:3, 3] = V @ v
    return T


class PoseBANumpy:
    """Localizer::DoLocalBA's cost from the definitions of its two edge types:
       sum_i huber(w_i |uv_i - project(T X_i)|^2) + e' Omega e,  e = log(meas T^-1) in (rotation, translation) order,
    huber(s) = s if s <= delta^2 else 2 delta sqrt(s) - delta^2 (g2o's RobustKernelHuber on the edge's chi2; none on the prior)."""

    def __init__(self, meas, info, X, uv, w, f, cx, cy, delta):
        self.meas = np.asarray(meas, float); self.info = np.asarray(info, float).reshape(6, 6)
        self.X = np.asarray(X, float).reshape(-1, 3); self.uv = np.asarray(uv, float).reshape(-1, 2)
        self.w = np.asarray(w, float).reshape(-1)
        self.f, self.cx, self.cy, self.delta = float(f), float(cx), float(cy), float(delta)
        lam, U = np.linalg.eigh(0.5 * (self.info + self.info.T))
        self.S = np.sqrt(np.clip(lam, 0, None))[:, None] * U.T     # Omega = S' S up to round-off: for the residual vector only

    def _parts(self, T):
        p = self.X @ T[:3, :3].T + T[:3, 3]
        r = self.uv - np.stack([self.f * p[:, 0] / p[:, 2] + self.cx, self.f * p[:, 1] / p[:, 2] + self.cy], 1)
        return r, se3_log_scipy(self.meas @ np.linalg.inv(T))

    def cost(self, T):
        r, e = self._parts(np.asarray(T, float))
        s = self.w * (r * r).sum(1)
        d2 = self.delta ** 2
        return float(np.where(s <= d2, s, 2 * self.delta * np.sqrt(s) - d2).sum() + e @ self.info @ e)

    def residuals(self, T):
        """vector whose squared norm is cost(T)"""
        r, e = self._parts(T)
        s = self.w * (r * r).sum(1)
        d2 = self.delta ** 2
        rho = np.where(s <= d2, s, 2 * self.delta * np.sqrt(np.maximum(s, 1e-300)) - d2)
        k = np.sqrt(self.w * rho / np.maximum(s, 1e-300))
        return np.concatenate([(r * k[:, None]).reshape(-1), self.S @ e])

    def minimise(self, T0):
        """scipy's trust-region least squares over d, T = exp(d) T0 -> (T, cost(T))"""
        from scipy.optimize import least_squares
        T0 = np.asarray(T0, float)
        sol = least_squares(lambda d: self.residuals(se3_exp_scipy(d) @ T0), np.zeros(6), jac="3-point", method="trf",
                            x_scale=np.array([1e-3] * 3 + [1.0] * 3), ftol=1e-15, xtol=1e-15, gtol=1e-13, max_nfev=400)
        T = se3_exp_scipy(sol.x) @ T0
        return T, self.cost(T)


def check_pose_ba(problem, Tcw0, T_out, stats, tol_final, margin):
    """problem: PoseBANumpy; T_out, stats: one implementation's result.  chi2_init / chi2_final equal the independent cost at
    the input / returned pose (1e-12 / tol_final relative); scipy started from the returned pose lowers the cost by at most
    `margin` (relative), and started from the input pose does not end lower than the result by more than `margin`.
    -> dict of the measured figures (relative)."""
    c0, c1 = problem.cost(Tcw0), problem.cost(T_out)
    assert np.isfinite(np.asarray(T_out)).all()
    d_init = abs(stats["chi2_init"] - c0) / c0
    d_final = abs(stats["chi2_final"] - c1) / c1
    assert d_init <= 1e-12, ("chi2_init", stats["chi2_init"], c0, d_init)
    assert d_final <= tol_final, ("chi2_final", stats["chi2_final"], c1, d_final)
    _, ca = problem.minimise(T_out)
    _, cb = problem.minimise(Tcw0)
    short_a, short_b = (c1 - ca) / c1, (c1 - cb) / c1
    assert short_a <= margin, ("scipy improves on the returned pose", c1, ca, short_a)
    assert short_b <= margin, ("scipy from the input pose ends lower", c1, cb, short_b)
    return dict(d_init=d_init, d_final=d_final, shortfall=max(short_a, short_b, 0.0))


def plane_motion_prior_numpy(Tcw, Tbc, xrot=1e6, yrot=1e6, zinfo=1.0):
    """addPlaneMotionSE3Expmap (optimizer.cpp:236-314) from its definition.  Measurement: the body pose T_bw = T_bc T_cw with
    height, roll and pitch removed (yaw = z component of the rotation vector... of the body rotation, translation (x, y, 0)),
    back in the camera frame.  Information: adj(T_bc)' diag(xrot, yrot, 1e-4, 1e-4, 1e-4, zinfo) adj(T_bc), the SE(3) adjoint in
    (rotation, translation) order: adj(T) = [[R, 0], [[t]x R, R]]; the upper triangle copied down (:296-298)."""
    from scipy.spatial.transform import Rotation
    Tcw = np.asarray(Tcw, float); Tbc = np.asarray(Tbc, float)
    Tbw = Tbc @ Tcw
    yaw = Rotation.from_matrix(Tbw[:3, :3]).as_rotvec()[2]
    M = np.eye(4)
    M[:3, :3] = Rotation.from_rotvec([0, 0, yaw]).as_matrix()
    M[:3, 3] = [Tbw[0, 3], Tbw[1, 3], 0.0]
    R, t = Tbc[:3, :3], Tbc[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R; A[3:, 3:] = R; A[3:, :3] = _hat(t) @ R
    info = A.T @ np.diag([xrot, yrot, 1e-4, 1e-4, 1e-4, zinfo]) @ A
    iu = np.triu_indices(6, 1)
    info[(iu[1], iu[0])] = info[iu]
    return np.linalg.inv(Tbc) @ M, info


# ------------------------------------------------------------------------------------------ fundamental-matrix RANSAC
def ransac_update_num_iters(p, ep, model_points, max_iters):
    """cv::RANSACUpdateNumIters (ptsetreg.cpp) written out: log(1 - p) / log(1 - (1 - ep)^model_points), rounded to nearest,
    never above max_iters; 0 when every point is an inlier"""
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = np.log(num), np.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def seven_point_numpy(x1, x2):
    """OpenCV's documented 7-point method on seven correspondences (7,2) f64: null space of the 7x9 system by numpy's SVD, the
    cubic det(l F1 + (1 - l) F2) by interpolation at four l and np.roots, the real roots, each F scaled to F[2,2] = 1
    -> list of 3x3"""
    A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1],
                  x1[:, 0], x1[:, 1], np.ones(7)], 1)
    if not np.isfinite(A).all():
        return []
    Vt = np.linalg.svd(A)[2]
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    ls = np.array([0.0, 1.0, -1.0, 2.0])
    dets = np.array([np.linalg.det(l * F1 + (1 - l) * F2) for l in ls])
    coef = np.linalg.solve(np.vander(ls, 4), dets)
    if not np.isfinite(coef).all() or not np.any(coef[:3]):
        return []
    out = []
    for r in np.roots(coef):
        if r.imag != 0:
            continue
        Fm = r.real * F1 + (1 - r.real) * F2
        if abs(Fm[2, 2]) > 2.220446049250313e-16:
            Fm = Fm / Fm[2, 2]
        out.append(Fm)
    return out


def epipolar_errors(F, p1, p2):
    """FMEstimatorCallback::computeError from its definition, FP64: err_i = max(d1^2 / (b0^2 + b1^2), d2^2 / (a0^2 + a1^2)) with
    a = F x1, b = F' x2, d2 = x2 . a, d1 = x1 . b; and per point a forward bound `dev` of what evaluating the same expression in
    float32 can move it by: a sum of k terms evaluated in float is off by at most (k + 1) u32 sum |terms| (products rounded,
    then added left to right), so  |dd| <= 8 u S_d  (nine products of three factors),  |da| <= 4 u S_a;  then
    d^2 / (a0^2 + a1^2) moves by at most  (2 |dd| |d| + err * 2 (|a0| da0 + |a1| da1)) / (a0^2 + a1^2) + 8 u err.
    F: (m,3,3); p1, p2: (n,2) -> err (m,n), dev (m,n)"""
    F = np.asarray(F, float).reshape(-1, 3, 3)
    x1 = np.c_[np.asarray(p1, float), np.ones(len(p1))]; x2 = np.c_[np.asarray(p2, float), np.ones(len(p2))]
    aF = np.abs(F)
    a = np.einsum("mij,nj->mni", F, x1); Sa = np.einsum("mij,nj->mni", aF, np.abs(x1))
    b = np.einsum("mji,nj->mni", F, x2); Sb = np.einsum("mji,nj->mni", aF, np.abs(x2))
    d2 = (a * x2).sum(2); Sd2 = (Sa * np.abs(x2)).sum(2)
    d1 = (b * x1).sum(2); Sd1 = (Sb * np.abs(x1)).sum(2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        na = a[..., 0] ** 2 + a[..., 1] ** 2; nb = b[..., 0] ** 2 + b[..., 1] ** 2
        e2 = d2 * d2 / na; e1 = d1 * d1 / nb
        v2 = (16 * U32 * Sd2 * np.abs(d2) + e2 * 8 * U32 * (np.abs(a[..., 0]) * Sa[..., 0] + np.abs(a[..., 1]) * Sa[..., 1])) / na + 8 * U32 * e2
        v1 = (16 * U32 * Sd1 * np.abs(d1) + e1 * 8 * U32 * (np.abs(b[..., 0]) * Sb[..., 0] + np.abs(b[..., 1]) * Sb[..., 1])) / nb + 8 * U32 * e1
    return np.maximum(e1, e2), np.maximum(v1, v2)


def fm_all_models(p1, p2, subsets):
    """the numpy 7-point models of every sample -> (F (M,3,3), sample index (M,)) in (sample, root) order"""
    x1 = np.asarray(p1, float); x2 = np.asarray(p2, float)
    Fs, its = [], []
    for it, idx in enumerate(subsets):
        for Fm in seven_point_numpy(x1[idx], x2[idx]):
            Fs.append(Fm); its.append(it)
    return np.array(Fs).reshape(-1, 3, 3), np.array(its, int)


def _match_model(Fs, F_impl):
    """index of the numpy model closest to the implementation's matrix, and the relative distance"""
    d = np.array([np.abs(Fm - F_impl).max() / np.abs(F_impl).max() for Fm in Fs])
    return int(np.argmin(d)), float(d.min())


def check_fundamental_mask(p1, p2, subsets, mask, n_inliers, info, F_winner):
    """findFundamentalMat's RANSAC mask (n >= 15) against an independent FP64 replay.  subsets: the samples the RNG draws (data);
    mask, n_inliers, info = {sample, model, iterations, inliers}: one implementation's answer; F_winner: the 7-point matrix
    that implementation computes for (sample, model), used only to find the same model among numpy's roots.
    -> dict(band share, matrix distance)"""
    p1 = np.asarray(p1, np.float32); p2 = np.asarray(p2, np.float32)
    n = len(p1)
    mask = np.asarray(mask).astype(bool)
    assert n >= 15 and mask.shape == (n,) and n_inliers == int(mask.sum()) == info["inliers"]
    s_w, R = info["sample"], info["iterations"]
    assert 0 <= s_w < len(subsets) and 0 <= R <= 1000
    Fs, its = fm_all_models(p1, p2, subsets)
    mine = np.flatnonzero(its == s_w)
    assert mine.size, "numpy finds no model for the reported sample"
    assert 0 <= info["model"] < 3
    k, dist = _match_model(Fs[mine], F_winner)
    assert dist <= 1e-6, "the winning matrix is %.2g (relative) away from every numpy root of that sample" % dist
    w = int(mine[k])
    lo = np.zeros(len(Fs), int); hi = np.zeros(len(Fs), int)
    for c in range(0, len(Fs), 256):
        err, dev = epipolar_errors(Fs[c:c + 256], p1, p2)
        lo[c:c + 256] = (err + dev < 9.0).sum(1)
        hi[c:c + 256] = (err - dev <= 9.0).sum(1)
        if c <= w < c + 256:
            e_w, d_w = err[w - c], dev[w - c]
    inside, outside = e_w + d_w < 9.0, e_w - d_w > 9.0
    band = ~(inside | outside)
    share = float(band.sum()) / n
    assert share <= 0.01, "%d of %d points within the float band of the threshold" % (band.sum(), n)
    assert mask[inside].all() and not mask[outside].any(), "mask differs from the FP64 inlier set outside the band"
    assert lo[w] <= n_inliers <= hi[w] and n_inliers > 6
    # RANSACPointSetRegistrator::run keeps the FIRST model that reaches the maximum
    order = np.arange(len(Fs))
    early = order < w
    assert not (lo[early] >= hi[w]).any(), "an earlier model has at least as many inliers"
    late = (order > w) & (its < R)
    assert not (lo[late] > hi[w]).any(), "a later model inside the loop has more inliers"
    # the loop bound only falls, and a model with g inliers implies a bound of at most f(g): the winner must lie inside
    # every bound the earlier models imply, and the final count is f(inliers of the winner)
    f = lambda g: ransac_update_num_iters(0.99, (n - g) / n, 7, 1000)
    for m in np.flatnonzero(early & (lo > 6)):
        assert s_w < f(int(lo[m])), "the loop had ended before the reported sample"
    assert f(int(hi[w])) <= R <= f(int(lo[w])), (f(int(hi[w])), R, f(int(lo[w])))
    return dict(band=share, dist=dist)


def check_lmeds_mask(p1, p2, subsets, mask, n_inliers, info, F_winner):
    """the LMedS branch (8 <= n <= 14): the winner's FP64 median is the first strict minimum over (sample, model) up to the band,
    the mask follows from sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median)"""
    p1 = np.asarray(p1, np.float32); p2 = np.asarray(p2, np.float32)
    n = len(p1)
    mask = np.asarray(mask).astype(bool)
    assert 8 <= n <= 14 and n_inliers == int(mask.sum()) == info["inliers"]
    assert info["iterations"] == len(subsets) == max(ransac_update_num_iters(0.99, 0.45, 7, 1000), 3)
    Fs, its = fm_all_models(p1, p2, subsets)
    mine = np.flatnonzero(its == info["sample"])
    assert mine.size
    k, dist = _match_model(Fs[mine], F_winner)
    assert dist <= 1e-6, dist
    w = int(mine[k])
    err, dev = epipolar_errors(Fs, p1, p2)
    srt = np.argsort(err, axis=1)
    rows = np.arange(len(Fs))
    pick = lambda a, j: a[rows, srt[:, j]]
    if n % 2:
        med, mdev = pick(err, n // 2), pick(dev, n // 2)
    else:
        med = 0.5 * (pick(err, n // 2 - 1) + pick(err, n // 2))
        mdev = 0.5 * (pick(dev, n // 2 - 1) + pick(dev, n // 2)) + 2 * U32 * med
    ok = np.isfinite(med)
    other = ok & (rows != w)
    assert not (med[other] + mdev[other] < med[w] - mdev[w]).any(), "another model has a smaller median"
    early = other & (rows < w)
    assert not (med[early] + mdev[early] <= med[w] - mdev[w]).any()
    c = (2.5 * 1.4826 * (1 + 5.0 / (n - 7))) ** 2
    thr, tdev = max(c * med[w], 1e-6), c * mdev[w] + 4 * U32 * c * med[w]
    inside, outside = err[w] + dev[w] < thr - tdev, err[w] - dev[w] > thr + tdev
    band = ~(inside | outside)
    assert band.sum() <= 0.01 * n, "%d of %d points within the float band of the threshold" % (band.sum(), n)
    assert mask[inside].all() and not mask[outside].any()
    return dict(band=float(band.sum()) / n, dist=dist)
