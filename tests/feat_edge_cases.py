"""Inputs of GlobalMapper::CreateFeatEdge for the tests, tools/feat_edge_bench.py and tools/fuzz_gpu.py: synth.kf_pair's two
key frames and common map points, measurements drawn around the true camera-frame points with covariance info^-1, a
perturbed start, planted outliers."""
import numpy as np

from se2lam_amd import synth


def make_pair(N, seed, kf_sigma=(15.0, 4e-3), mp_sigma=30.0, n_outliers=0, turn_y=0.0):
    """-> dict(kf (2,4,4) start poses, mp (N,3) start points, z (N,2,3), info (N,2,3,3), planted (N,) bool).
    Key frame 1 starts about kf_sigma[0] mm and kf_sigma[1] rad off (and turned by turn_y rad about its camera's y axis:
    a start that makes Levenberg-Marquardt reject trials), the points about mp_sigma mm off.  A planted outlier has its
    measurement in key frame 1 shifted by 60 mm in x: the depth sigma of kf_pair is hundreds of mm, so only a lateral
    shift is one."""
    kf, mp, _, _, m_info = synth.kf_pair(N, seed)
    info = m_info.reshape(N, 2, 3, 3)
    rng = np.random.default_rng(77000 + seed)
    z = np.zeros((N, 2, 3))
    for j in range(N):
        for k in range(2):
            zc = kf[k][:3, :3].T @ (mp[j] - kf[k][:3, 3])
            z[j, k] = zc + np.linalg.cholesky(np.linalg.inv(info[j, k])) @ rng.normal(0, 1, 3)
    planted = np.zeros(N, bool)
    if n_outliers:
        planted[rng.choice(N, n_outliers, replace=False)] = True
        z[planted, 1, 0] += 60.0
    start = kf.copy()
    d = np.concatenate([rng.normal(0, kf_sigma[0] / np.sqrt(3), 3), rng.normal(0, 0.5 * kf_sigma[1] / np.sqrt(3), 3)])   # angle = 2 |q|
    start[1] = kf[1] @ synth.from_mqt_np(d)
    if turn_y:
        c, s = np.cos(turn_y), np.sin(turn_y)
        Ty = np.eye(4)
        Ty[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        start[1] = start[1] @ Ty
    mp0 = mp + rng.normal(0, mp_sigma / np.sqrt(3), (N, 3))
    return dict(kf=start, mp=mp0, z=z, info=info, planted=planted, kf_true=kf, mp_true=mp)


# (N, seed): the minimum of each mode (3 matches / 10 covisible points), the lane boundary on both sides, three strides with a
# tail.  Seeds chosen on the CPU model so that no edge chi2 of a match-mode case lies within 1e-3 relative of the threshold.
MATCH_SHAPES = ((3, 0), (10, 0), (63, 0), (64, 0), (65, 0), (130, 0))
COVIS_SHAPES = ((10, 0), (63, 0), (64, 0), (65, 0), (130, 0))
OUTLIER_CASES = ((40, 0, 5), (65, 1, 9))          # (N, seed, planted): seeds at which the model rejects every planted point
# key frame 1 turned by 2.2 rad about its camera's y axis, key frame 0 fixed, 14 iterations: the model's trial history ends
# ... 3, 3, 2 while chi2 is still falling fast (genuine rejections, not rounding)
REJECTING = dict(N=12, seed=1, turn_y=2.2, iters=14)


def with_camera(c, Tbc):
    """the pair c as a camera mounted at Tbc (4x4) on the same body sees it: T_w_c' = T_w_c T_c_c' with T_c_c' = Tbc_old^-1 Tbc, the
    measurements and their informations turned into the new camera frame; points, noise draws and planted outliers stay"""
    D = np.linalg.inv(synth.tbc44()) @ np.asarray(Tbc, np.float64)
    R, t = D[:3, :3], D[:3, 3]
    out = dict(c, kf=c["kf"] @ D, z=(c["z"] - t) @ R, info=np.einsum("ji,nkjl,lm->nkim", R, c["info"], R))
    if "kf_true" in c:
        out["kf_true"] = c["kf_true"] @ D
    return out


def as_tuple(c):
    return c["kf"], c["mp"], c["z"], c["info"]


def empty_pair(seed=0):
    """two key frames without a common point"""
    kf = synth.kf_pair(3, seed)[0]
    return dict(kf=kf, mp=np.zeros((0, 3)), z=np.zeros((0, 2, 3)), info=np.zeros((0, 2, 3, 3)), planted=np.zeros(0, bool))
