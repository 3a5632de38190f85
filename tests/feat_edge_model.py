"""Independent FP64 model of the two-key-frame bundle adjustment of GlobalMapper::CreateFeatEdge
(/root/reference/src/GlobalMapper.cpp:847-1032): g2o::VertexSE3 + EdgeSE3Prior + VertexPointXYZ + EdgeSE3PointXYZ (Huber),
as a DENSE Levenberg-Marquardt over the full 12 + 3 N system - no Schur complement, numpy.linalg.solve - with g2o's controller
(oracle/pg_ref.cpp:300-351).  It shares no code with csrc/feat_edge.hip: poses are 4x4 matrices, quaternions come from scipy
(synth.mqt_np / from_mqt_np), the prior from synth.plane_motion_prior_se3_np."""
import numpy as np

from se2lam_amd import synth

COVIS, MATCH = 0, 1


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def huber(e2, delta):
    """RobustKernelHuber: (rho, rho')"""
    if e2 <= delta * delta:
        return e2, 1.0
    s = np.sqrt(e2)
    return 2 * s * delta - delta * delta, delta / s


def edge_error(T, p, z):
    """EdgeSE3PointXYZ with the identity offset: the point in the camera frame minus the measurement"""
    return T[:3, :3].T @ (p - T[:3, 3]) - z


def edge_jacobians(T, p):
    """(d e / d pose update (translation, compact quaternion), d e / d point)"""
    zc = T[:3, :3].T @ (p - T[:3, 3])
    return np.hstack([-np.eye(3), 2 * skew(zc)]), T[:3, :3].T


def oplus_pose(T, d):
    return T @ synth.from_mqt_np(d)       # VertexSE3::oplusImpl (rotation = identity when |q|^2 > 1)


def mqt_eigen(T):
    """g2o::internal::toVectorMQT on a matrix block that need not be a rotation: Eigen::Quaterniond(M) as Eigen's
    quaternionbase_assign_impl defines it (the trace, or the largest diagonal entry i with j = i + 1, k = j + 1 cyclically), then
    normalize() and w >= 0.  The key frames of a map are float tables: their rotation blocks are 4e-8 away from orthonormal, and on
    such a matrix scipy's conversion (synth.mqt_np) answers another question - its quaternion differs from Eigen's by that 4e-8
    times the rotation's own size, which is 1e-11 of the cost of a ten-point pair under a tilted extrinsic."""
    m = np.asarray(T, np.float64)[:3, :3]
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)                                   # w, x, y, z
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1:] = [(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    return np.concatenate([np.asarray(T)[:3, 3], q[1:]])


def prior_error(Z, T):
    return mqt_eigen(np.linalg.inv(Z) @ T)


def prior_jacobian(Z, T):
    """d toVectorMQT(Z^-1 T fromVectorMQT(d)) / d d at 0: [R_E 0; 0 w_E I + [q_E]x]"""
    E = np.linalg.inv(Z) @ T
    q = synth.mqt_np(E)[3:]
    w = np.sqrt(max(0.0, 1 - q @ q))
    J = np.zeros((6, 6))
    J[:3, :3] = E[:3, :3]
    J[3:, 3:] = w * np.eye(3) + skew(q)
    return J


class Problem:
    """kf (2,4,4) T_w_c, mp (N,3), z (N,2,3), info (N,2,3,3); the priors are built from the INPUT poses"""

    def __init__(self, kf, mp, z, info, mode, huber_delta=5.99, prior_kw=None):
        self.kf0 = np.array(kf, np.float64)
        self.mp0 = np.array(mp, np.float64).reshape(-1, 3)
        self.z = np.asarray(z, np.float64).reshape(-1, 2, 3)
        self.W = np.asarray(info, np.float64).reshape(-1, 2, 3, 3)
        self.N = len(self.mp0)
        self.fixed0 = mode == COVIS
        self.delta = huber_delta
        self.prior = [synth.plane_motion_prior_se3_np(self.kf0[k], **(prior_kw or {})) for k in range(2)]

    def _errors(self, T, mp, k):
        """all edges of key frame k at once (the suite runs this model for every case): (z_c, e, e' W e)"""
        zc = (mp - T[:3, 3]) @ T[:3, :3]
        e = zc - self.z[:, k]
        return zc, e, np.einsum("ni,nij,nj->n", e, self.W[:, k], e)

    def edge_chi2(self, kf, mp):
        return np.stack([self._errors(kf[k], mp, k)[2] for k in range(2)], axis=1) if self.N else np.zeros((0, 2))

    def cost(self, kf, mp):
        c = sum(huber(v, self.delta)[0] for v in self.edge_chi2(kf, mp).ravel())
        for k in range(2):
            e = prior_error(self.prior[k][0], kf[k])
            c += e @ self.prior[k][1] @ e
        return c

    def system(self, kf, mp):
        """H, b of the whole graph (edge_jacobians, for every edge of a key frame at once)"""
        n = 12 + 3 * self.N
        H, b = np.zeros((n, n)), np.zeros(n)
        for k in range(2 if self.N else 0):
            zc, e, chi = self._errors(kf[k], mp, k)
            W = self.W[:, k] * np.array([huber(v, self.delta)[1] for v in chi])[:, None, None]
            Jp = np.zeros((self.N, 3, 6))
            Jp[:, :, :3] = -np.eye(3)
            Jp[:, 0, 4], Jp[:, 0, 5] = -2 * zc[:, 2], 2 * zc[:, 1]
            Jp[:, 1, 3], Jp[:, 1, 5] = 2 * zc[:, 2], -2 * zc[:, 0]
            Jp[:, 2, 3], Jp[:, 2, 4] = -2 * zc[:, 1], 2 * zc[:, 0]
            Jl = kf[k][:3, :3].T
            sp = slice(6 * k, 6 * k + 6)
            H[sp, sp] += np.einsum("nri,nrs,nsj->ij", Jp, W, Jp)
            b[sp] -= np.einsum("nri,nrs,ns->i", Jp, W, e)
            Hpl = np.einsum("nri,nrs,sj->nij", Jp, W, Jl)
            Hll = np.einsum("ri,nrs,sj->nij", Jl, W, Jl)
            bl = np.einsum("ri,nrs,ns->ni", Jl, W, e)
            for j in range(self.N):
                sl = slice(12 + 3 * j, 15 + 3 * j)
                H[sp, sl] += Hpl[j]
                H[sl, sp] += Hpl[j].T
                H[sl, sl] += Hll[j]
                b[sl] -= bl[j]
        for k in range(2):
            Z, W = self.prior[k]
            J, e = prior_jacobian(Z, kf[k]), prior_error(Z, kf[k])
            sp = slice(6 * k, 6 * k + 6)
            H[sp, sp] += J.T @ W @ J
            b[sp] -= J.T @ W @ e
        return H, b

    def free(self):
        f = np.ones(12 + 3 * self.N, bool)
        if self.fixed0:
            f[:6] = False
        return f

    def apply(self, kf, mp, x):
        kf2 = kf.copy()
        for k in range(2):
            if not (k == 0 and self.fixed0):
                kf2[k] = oplus_pose(kf[k], x[6 * k:6 * k + 6])
        return kf2, mp + x[12:].reshape(-1, 3)


def optimize(pb: Problem, iters, outlier_chi2=5.0):
    """-> dict(kf, mp, chi2_init, chi2_hist, lambda_hist, trials_hist, terminated, edge_chi2, outlier, update)"""
    kf, mp = pb.kf0.copy(), pb.mp0.copy()
    free = pb.free()
    chi = pb.cost(kf, mp)
    out = dict(chi2_init=chi, chi2_hist=[], lambda_hist=[], trials_hist=[], terminated=0)
    lam, ni = 0.0, 2.0
    for it in range(iters):
        H, b = pb.system(kf, mp)
        if it == 0:
            lam, ni = 1e-5 * np.abs(np.diag(H)[free]).max(), 2.0
        rho, qmax = 0.0, 0
        while True:
            F = H[np.ix_(free, free)] + lam * np.eye(int(free.sum()))
            x = np.zeros(len(b))
            ok = True
            try:
                np.linalg.cholesky(F)
                x[free] = np.linalg.solve(F, b[free])
            except np.linalg.LinAlgError:
                ok = False
            kt, mt = pb.apply(kf, mp, x)
            scale = float(np.sum(x[free] * (lam * x[free] + b[free])))
            tchi = pb.cost(kt, mt) if ok else np.finfo(float).max
            qmax += 1
            rho = (chi - tchi) / (scale + 1e-3)
            if rho > 0 and np.isfinite(tchi):
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                ni = 2.0
                chi, kf, mp = tchi, kt, mt
            else:
                lam *= ni
                ni *= 2
            if not (rho < 0 and qmax < 10):
                break
        out["chi2_hist"].append(chi)
        out["lambda_hist"].append(lam)
        out["trials_hist"].append(qmax)
        if qmax == 10 or rho == 0:
            out["terminated"] = 1
            break
    ec = pb.edge_chi2(kf, mp)
    reject = (not pb.fixed0) and outlier_chi2 > 0
    out.update(kf=kf, mp=mp, edge_chi2=ec, outlier=(ec > outlier_chi2).any(axis=1) if reject else np.zeros(pb.N, bool),
               update=max(np.abs(kf - pb.kf0).max(), np.abs(mp - pb.mp0).max() if pb.N else 0.0),
               chi2_hist=np.array(out["chi2_hist"]), lambda_hist=np.array(out["lambda_hist"]), trials_hist=np.array(out["trials_hist"]))
    return out


def compared_prefix(chi2_init, chi2_hist, trials_hist=None):
    """the number of leading iterations whose accepted step lowers the model's chi2 by more than 1e-8 relative: beyond it,
    accepting or rejecting a trial is decided by rounding, and the LM history is not compared"""
    prev, n = chi2_init, 0
    for c in chi2_hist:
        if not (prev - c > 1e-8 * prev):
            break
        prev, n = c, n + 1
    return n


REL = 1e-5


def inputs_ok(m, mode, outlier_chi2=5.0):
    """the conditions on a case, on the model alone: a compared prefix of at least 10 iterations, no edge chi2 within 1e-3
    relative of the rejection threshold"""
    n = compared_prefix(m["chi2_init"], m["chi2_hist"])
    return n >= 10 and (mode == COVIS or not m["edge_chi2"].size or np.abs(m["edge_chi2"] - outlier_chi2).min() > 1e-3 * outlier_chi2)


def check_against_model(got, c, m, mode, oracle, label):
    """THE comparison of a device result (se2lam_amd.feat_edge.CreateFeatEdgeBatch, one pair) with this model's, and of its
    sparsifier stage with oracle.sparsify fed the device's own poses and inliers - tests/test_feat_edge_gpu.py and
    tools/fuzz_gpu.py both call it.  Prints each figure before it asserts."""
    s = got["stats"]
    N = len(c["mp"])
    assert got["status"] == 0 and got["n_points"] == N
    print("%s: chi2 %.6g -> %.6g (model %.6g -> %.6g), trials %s" % (label, s["chi2_init"], s["chi2_final"], m["chi2_init"],
                                                                      m["chi2_hist"][-1], s["trials_hist"].tolist()))
    assert np.isclose(s["chi2_init"], m["chi2_init"], rtol=1e-11, atol=0)
    n = compared_prefix(m["chi2_init"], m["chi2_hist"])
    assert n >= 10 and s["iterations"] >= n
    assert np.allclose(s["chi2_hist"][:n], m["chi2_hist"][:n], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"][:n], m["lambda_hist"][:n], rtol=REL, atol=0)
    assert np.array_equal(s["trials_hist"][:n], m["trials_hist"][:n])
    dev = max(np.abs(got["kf"] - m["kf"]).max(), np.abs(got["mp"] - m["mp"]).max())
    print("%s: final state off the model by %.3g, the model's largest update %.3g" % (label, dev, m["update"]))
    assert dev <= REL * m["update"]
    if mode == COVIS:
        assert np.array_equal(got["kf"][0], c["kf"][0])
    assert np.allclose(got["edge_chi2"], m["edge_chi2"], rtol=1e-4, atol=1e-7)
    if mode == MATCH:
        assert np.abs(m["edge_chi2"] - 5.0).min() > 1e-3 * 5.0       # the condition on the inputs
    assert np.array_equal(got["outlier"], m["outlier"])
    assert got["n_outliers"] == int(m["outlier"].sum()) and got["n_sparsified"] == N - got["n_outliers"]
    # the sparsifier stage on the device's own result: the chaining and the compaction, in input order
    keep = ~got["outlier"]
    ni = int(keep.sum())
    m_kf, m_mp = np.tile([0, 1], ni).astype(np.int32), np.repeat(np.arange(ni), 2).astype(np.int32)
    zr, ir, _ = oracle.sparsify(got["kf"], got["mp"][keep], m_kf, m_mp, c["info"][keep].reshape(-1, 3, 3))
    assert np.allclose(got["z"], zr, atol=1e-12)
    assert np.abs(got["info"] - ir).max() <= REL * np.abs(ir).max()
    assert np.abs(got["info"] - got["info"].T).max() == 0
    # end to end (model -> oracle.sparsify): reported, not a criterion - the step is ill-conditioned by construction
    zm, im, _ = oracle.sparsify(m["kf"], m["mp"][m["outlier"] == 0], m_kf, m_mp, c["info"][keep].reshape(-1, 3, 3))
    print("%s: end to end against model -> oracle.sparsify: z %.3g, info %.3g of its largest entry"
          % (label, np.abs(got["z"] - zm).max(), np.abs(got["info"] - im).max() / np.abs(im).max()))
