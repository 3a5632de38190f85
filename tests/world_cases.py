"""The 6-DoF graphs of synth in a rotated world.  Every vertex the generators make is se2_to_Tcw(planar pose) times milliradians
of noise: all rotations share one axis, and whatever a kernel gets wrong about a general rotation is zero or symmetric on them.
G below is a fixed rigid motion of the world, 2.37 rad about an axis that is no coordinate axis plus metres of translation; a
problem moved by it has the same cost, the same reduced system up to the change of the landmarks' frame, and the same
Levenberg-Marquardt history, while no rotation matrix in it has a zero entry.  No tests, no fixtures: the modules that use it
are test_rotated_world.py (CPU) and test_rotated_world_gpu.py."""
import dataclasses

import numpy as np
from scipy.spatial.transform import Rotation

from se2lam_amd import synth

G = np.eye(4)
# The rotation vector (2.37 rad) was searched once, over vectors of 2.0 to 2.4 rad with three decimals, for the two properties
# test_rotated_world.py asserts of every case in CASES_*: the moved key frames take all four branches of quat_of, and no entry of
# a moved vertex rotation is below 0.02 in magnitude.
G[:3, :3] = Rotation.from_rotvec([-1.424, 1.689, -0.862]).as_matrix()
G[:3, 3] = [1500.0, -2300.0, 900.0]                                                     # mm


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def move_pose_graph(g, M=G):
    """VertexSE3 holds T_w_c: the world moved by M turns it into M T_w_c, and the plane-motion measurements with it.  The errors
    toVectorMQT(Z^-1 X_i^-1 X_j) and toVectorMQT(meas^-1 X) do not change, so the EdgeSE3 measurements and every information stay."""
    return dataclasses.replace(g, poses=M @ g.poses, prior_meas=M @ g.prior_meas,
                               poses_true=None if g.poses_true is None else M @ g.poses_true)


def pose_graph_back(X, M=G):
    return inv(M) @ X


def move_ba3(g, M=G):
    """VertexSE3Expmap holds T_c_w: T_c_w M^-1, landmarks M X, so that T X is unchanged (oracle/ba3_ref.cpp: the projection edge).
    EdgeSE3ExpmapPrior's error log(meas T^-1) keeps its value with meas M^-1, and its information.  EdgeSE3Expmap's error
    log(T_j^-1 C T_i) becomes log(M (T_j^-1 C T_i) M^-1) = Adj(M) log(T_j^-1 C T_i): C stays and the information becomes
    Adj(M)^-T W Adj(M)^-1 (Adj in the order (omega, upsilon), synth.se3_adj_np), symmetrised after the two products."""
    Mi = inv(M)
    Ai = np.linalg.inv(synth.se3_adj_np(M))
    W = np.einsum("ji,ojk,kl->oil", Ai, g.o_info, Ai)
    return dataclasses.replace(g, poses=g.poses @ Mi, lms=g.lms @ M[:3, :3].T + M[:3, 3], prior_meas=g.prior_meas @ Mi,
                               o_info=0.5 * (W + W.transpose(0, 2, 1)),
                               poses_true=None if g.poses_true is None else g.poses_true @ Mi)


def ba3_back(poses, lms, M=G):
    """estimates of a moved SE3 window in the original world: (P,4,4) and (L,3)"""
    return poses @ M, (lms - M[:3, 3]) @ M[:3, :3]


def pose44(p12):
    p12 = np.asarray(p12)
    T = np.zeros(p12.shape[:-1] + (4, 4))
    T[..., 3, 3] = 1
    T[..., :3, :3] = p12[..., :9].reshape(p12.shape[:-1] + (3, 3))
    T[..., :3, 3] = p12[..., 9:]
    return T


def quat_branch(R):
    """the branch Eigen's matrix-to-quaternion conversion takes (quat_of / normalize_rotation of csrc/se3_math.h): 0 for a positive
    trace, else 1 + the index of the largest diagonal entry, the first of equal ones"""
    R = np.asarray(R)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def census(poses):
    """(how many of the rotations take each of the four branches, the smallest |entry| of any of them)"""
    R = np.asarray(poses)[:, :3, :3]
    return np.bincount([quat_branch(r) for r in R], minlength=4), float(np.abs(R).min())


def seam_ring(P=6, seed=0, step=0.25):
    """A pose graph as synth.pose_graph makes it - drifted start, plane-motion priors, odometry edges (a + 1, a), feature edges two
    and three ahead - of P key frames whose headings are centred on pi: pi + step (a - (P - 1) / 2).  synth.pose_graph keeps every
    heading inside (-pi + 0.1, pi - 0.1); here the body's yaw, as the plane-motion prior takes it from a quaternion, changes sign
    between the two middle key frames."""
    rng = np.random.default_rng([seed, P, 31415])
    head = np.pi + step * (np.arange(P) - 0.5 * (P - 1))
    ang = head - np.pi / 2
    se2 = np.stack([6000.0 * np.cos(ang), 6000.0 * np.sin(ang), head], axis=1)
    true = np.stack([inv(synth.se2_to_Tcw(p)) for p in se2])
    poses = true.copy()
    drift = np.eye(4)
    for a in range(1, P):
        drift = drift @ synth.from_mqt_np(rng.normal(0, 1.0, 6) * np.array([4.0, 4.0, 0.5, 2e-4, 2e-4, 8e-4]))
        poses[a] = true[a] @ drift
    fixed = np.zeros(P, np.uint8)
    fixed[0] = 1
    pm = [synth.plane_motion_prior_se3_np(poses[a]) for a in range(P)]
    oi, oj, om, ow = [], [], [], []

    def add(i, j, sig_t, sig_r):
        Z = inv(true[i]) @ true[j] @ synth.from_mqt_np(rng.normal(0, 1.0, 6) * np.array([sig_t] * 3 + [sig_r] * 3))
        A = np.diag([1 / sig_t ** 2] * 3 + [1 / sig_r ** 2] * 3)
        B = rng.normal(0, 1, (6, 6)) * 0.05
        S = np.diag(np.sqrt(np.diag(A)))
        W = A + S @ (B + B.T) @ S
        assert np.linalg.eigvalsh(W).min() > 0
        oi.append(i); oj.append(j); om.append(Z); ow.append(W)

    for a in range(P - 1):
        add(a + 1, a, 3.0, 1e-3)
    for a in range(P):
        for d in (2, 3):
            if a + d < P:
                add(a, a + d, 8.0, 2e-3)
    return synth.PoseGraph(poses=poses, fixed=fixed, has_prior=np.ones(P, np.uint8), prior_meas=np.stack([m for m, _ in pm]),
                           prior_info=np.stack([w for _, w in pm]), o_i=np.array(oi, np.int32), o_j=np.array(oj, np.int32),
                           o_meas=np.stack(om), o_info=np.stack(ow), poses_true=true), head


# ---- the cases: name -> the graph in the generator's world.  Small on purpose: 6 to 21 key frames.
PG_REJECTING = (12, 4, 55)            # pg_cases.REJECTING[1]


def pg_case(name):
    import pg_cases
    if name == "rejecting":
        return pg_cases.rejecting(*PG_REJECTING)
    return synth.pose_graph(int(name[1:]))


def ba3_case(name):
    from ba_cases import REJECT, kidnapped3
    if name == "reject":
        return kidnapped3(synth, *REJECT)
    return {"8": synth.ba3_graph(8, 60), "21": synth.ba3_graph(21, 600, n_ref=3)}[name]


PG_CASES = ("P6", "P17", "rejecting")
BA3_CASES = ("8", "21", "reject")
