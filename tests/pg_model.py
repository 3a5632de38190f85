"""A numpy / scipy model of the pose-graph cost (GlobalMapper::GlobalBA: EdgeSE3Prior e = toVectorMQT(M^-1 X), EdgeSE3
e = toVectorMQT(Z^-1 X_i^-1 X_j), vertex update X <- X * fromVectorMQT(d)) that shares no formula with oracle/pg_ref.cpp or
csrc/se3_math.h: rotations go through scipy's quaternions, and the normal equations H = sum J' W J, b = -sum J' W e come from
central differences of the error itself - no Jacobian is written down anywhere in this file."""
import numpy as np
from scipy.spatial.transform import Rotation


def mqt(T):
    """(translation, vector part of the unit quaternion with w >= 0)"""
    q = Rotation.from_matrix(T[:3, :3]).as_quat()      # (x, y, z, w)
    if q[3] < 0:
        q = -q
    return np.concatenate([T[:3, 3], q[:3]])


def from_mqt(d):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat([d[3], d[4], d[5], np.sqrt(1.0 - d[3:] @ d[3:])]).as_matrix()
    T[:3, 3] = d[:3]
    return T


def _inv(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ t
    return out


def prior_error(M, X):
    return mqt(_inv(M) @ X)


def edge_error(Z, Xi, Xj):
    return mqt(_inv(Z) @ _inv(Xi) @ Xj)


def cost(g, X):
    """-> (sum over the priors and edges of e' W e, the edges' terms in the order they were added).  Priors of fixed key
    frames count as g2o counts them: an EdgeSE3Prior on a fixed vertex is still an active edge."""
    chi, ec = 0.0, np.zeros(g.O)
    for a in range(g.P):
        if g.has_prior[a]:
            e = prior_error(g.prior_meas[a], X[a])
            chi += e @ g.prior_info[a] @ e
    for k in range(g.O):
        e = edge_error(g.o_meas[k], X[g.o_i[k]], X[g.o_j[k]])
        ec[k] = e @ g.o_info[k] @ e
    return chi + ec.sum(), ec


H_STEP = 1e-3


def _jac(f, X):
    """d f(X * from_mqt(d)) / d d at 0 by the five-point central difference with step H_STEP (truncation h^4 / 30 f^(5),
    round-off eps |f| / h: both near 1e-12 of the largest entry on these graphs)"""
    J = np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = H_STEP
        f1 = f(X @ from_mqt(d)) - f(X @ from_mqt(-d))
        f2 = f(X @ from_mqt(2 * d)) - f(X @ from_mqt(-2 * d))
        J[:, c] = (8.0 * f1 - f2) / (12.0 * H_STEP)
    return J


def system(g, X):
    """H (6P, 6P) and b (6P) of the Gauss-Newton step at X, lambda = 0.  Fixed key frames are left out: their rows and columns
    stay zero.  A slot's block is the sum over its edges simply because every edge adds into the same place."""
    n = 6 * g.P
    H, b = np.zeros((n, n)), np.zeros(n)
    free = ~np.asarray(g.fixed, bool)
    for a in range(g.P):
        if g.has_prior[a] and free[a]:
            W, s = g.prior_info[a], slice(6 * a, 6 * a + 6)
            J = _jac(lambda Y: prior_error(g.prior_meas[a], Y), X[a])
            H[s, s] += J.T @ W @ J
            b[s] -= J.T @ W @ prior_error(g.prior_meas[a], X[a])
    for k in range(g.O):
        i, j, Z, W = int(g.o_i[k]), int(g.o_j[k]), g.o_meas[k], g.o_info[k]
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        e = edge_error(Z, X[i], X[j])
        Ji = _jac(lambda Y: edge_error(Z, Y, X[j]), X[i]) if free[i] else None
        Jj = _jac(lambda Y: edge_error(Z, X[i], Y), X[j]) if free[j] else None
        if free[i]:
            H[si, si] += Ji.T @ W @ Ji
            b[si] -= Ji.T @ W @ e
        if free[j]:
            H[sj, sj] += Jj.T @ W @ Jj
            b[sj] -= Jj.T @ W @ e
        if free[i] and free[j]:
            H[si, sj] += Ji.T @ W @ Jj
            H[sj, si] += Jj.T @ W @ Ji
    return H, b


def free_mask(g):
    return np.repeat(~np.asarray(g.fixed, bool), 6)


def distance(g, H, b, Hm, bm):
    """(max |H - Hm| / max |Hm|, max |b - bm| / max |bm|) over the free key frames"""
    f = free_mask(g)
    return (np.abs(H[f][:, f] - Hm[f][:, f]).max() / np.abs(Hm[f][:, f]).max(), np.abs(b[f] - bm[f]).max() / np.abs(bm[f]).max())


def scaled_distance(g, H, b, Hm, bm):
    """`distance` in the system's own scale (tests/scaled_parity.py): every entry over d_i d_j, d = sqrt(diag(Hm)), so that the
    translation entries are not measured against the rotation entries' 1e6"""
    import scaled_parity as sp
    f = free_mask(g)
    return sp.scaled_distance(H[f][:, f], Hm[f][:, f]), sp.scaled_rhs_distance(b[f], bm[f], Hm[f][:, f])
