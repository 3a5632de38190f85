"""Pose graphs (GlobalMapper::GlobalBA: VertexSE3 + EdgeSE3Prior + EdgeSE3) beyond the ring synth.pose_graph makes, and starts on
which Levenberg-Marquardt rejects trials.  Every case keeps the generator's start, truth and plane-motion priors and draws its
own EdgeSE3 set the way the generator's `add` does: noise on true_i^-1 true_j, an SPD information with small off-diagonals.
tests/test_pg_model.py holds the cases to their conditions on the CPU (SPD, condition number, a history that does not hang
on a decision), so that a failure of tests/test_pg_layouts_gpu.py means the kernels."""
import dataclasses
import functools
import os

import numpy as np

from se2lam_amd import synth

SIG_T, SIG_R = 5.0, 1.5e-3        # mm / quaternion-vector units: between the generator's odometry and feature edges

# kind -> the smallest P at which the layout is what its row says
KINDS = {
    "chain_no_priors": 2,   # edges (a+1, a), no EdgeSE3Prior at all: prior_has == 0 for every key frame
    "sparse_priors": 2,     # the chain; key frames 2, 5, 8 ... lose their prior: ph / pb zero and non-zero side by side
    "multi_fixed": 5,       # 0, P//2, P-1 fixed: a fixed i, a fixed j, slots between two fixed key frames (in chi2, not in H)
    "slots": 3,             # the chain plus (0,1),(1,0),(0,1), (a,a+1) for odd a < P-2, (P-1,P-2) twice: slots of 4 (at the fixed
                            # key frame 0), 2 (both orientations) and 3 edges
    "star": 2,              # every key frame joined to 0 only, orientation alternating, no priors
    "upper_only": 2,        # (a, a+1) and (a, a+2): no edge with i > j
    "components": 4,        # two chains without an edge between them: the second is held by its priors
    "complete": 2,          # every pair, orientation by the parity of a + b: nothing for nested dissection to cut
    "shuffled": 2,          # the generator's own edges in a random order: pg_perm, the per-edge chi2 order
}


def _pairs(kind, P):
    chain = [(a + 1, a) for a in range(P - 1)]
    if kind in ("chain_no_priors", "sparse_priors"):
        return chain
    if kind == "multi_fixed":
        return chain + [(0, P - 1), (P - 1, P // 2), (P // 2, 1)]
    if kind == "slots":
        return chain + [(0, 1), (1, 0), (0, 1)] + [(a, a + 1) for a in range(1, P - 2, 2)] + [(P - 1, P - 2)] * 2
    if kind == "star":
        return [(a, 0) if a % 2 else (0, a) for a in range(1, P)]
    if kind == "upper_only":
        return [(a, a + d) for a in range(P) for d in (1, 2) if a + d < P]
    if kind == "components":
        h = P // 2
        return [(a + 1, a) for a in range(h - 1)] + [(a + 1, a) for a in range(h, P - 1)]
    if kind == "complete":
        return [(a, b) if (a + b) % 2 else (b, a) for a in range(P) for b in range(a + 1, P)]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def layout(kind: str, P: int, seed: int = 0) -> "synth.PoseGraph":
    assert P >= KINDS[kind], (kind, P)
    base = synth.pose_graph(P)
    rng = np.random.default_rng(1000 * seed + 31 * P + list(KINDS).index(kind))
    fixed, has_prior = base.fixed.copy(), base.has_prior.copy()
    if kind == "shuffled":
        order = rng.permutation(base.O)
        if np.array_equal(order, np.arange(base.O)):        # (two edges at P = 2)
            order = np.roll(order, 1)
        return dataclasses.replace(base, o_i=base.o_i[order].copy(), o_j=base.o_j[order].copy(), o_meas=base.o_meas[order].copy(),
                                   o_info=base.o_info[order].copy())
    if kind in ("chain_no_priors", "star"):
        has_prior[:] = 0
    if kind == "sparse_priors":
        has_prior[2::3] = 0
    if kind == "multi_fixed":
        fixed[[0, P // 2, P - 1]] = 1
    true = base.poses_true
    oi, oj, om, ow = [], [], [], []
    for i, j in _pairs(kind, P):
        Z = np.linalg.inv(true[i]) @ true[j] @ synth.from_mqt_np(rng.normal(0, 1.0, 6) * np.array([SIG_T] * 3 + [SIG_R] * 3))
        A = np.diag([1 / SIG_T ** 2] * 3 + [1 / SIG_R ** 2] * 3)
        B = rng.normal(0, 1, (6, 6)) * 0.05
        S = np.diag(np.sqrt(np.diag(A)))
        W = A + S @ (B + B.T) @ S
        assert np.linalg.eigvalsh(W).min() > 0
        oi.append(i); oj.append(j); om.append(Z); ow.append(W)
    return dataclasses.replace(base, fixed=fixed, has_prior=has_prior, o_i=np.array(oi, np.int32), o_j=np.array(oj, np.int32),
                               o_meas=np.stack(om), o_info=np.stack(ow))


def kinds_at(P: int):
    return [k for k, pmin in KINDS.items() if P >= pmin]


# (P, nbad, seed): nbad key frames of synth.pose_graph(P) turned by almost 180 degrees about a random axis.  Translations alone
# never make LM reject a trial on these graphs; a half turn does.  tests/test_pg_model.py::test_rejecting_starts_* decides
# which triples may stand here: (12, 4, 8) rejected nothing with these draws and gave way to (12, 4, 55); the oracle's histories
# are [1, 1, 6, 1, 1, 1, 1, 1, 1, 1] (minimum |rho| 5.4e-3) and [1, 1, 1, 1, 1, 1, 1, 7, 1, 1] (3.3e-3).
REJECTING = [(24, 1, 7), (12, 4, 55)]


@functools.lru_cache(maxsize=None)
def rejecting(P: int, nbad: int, seed: int) -> "synth.PoseGraph":
    base = synth.pose_graph(P)
    rng = np.random.default_rng(seed)
    poses = base.poses.copy()
    for a in rng.choice(np.arange(1, P), nbad, replace=False):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        poses[a] = poses[a] @ synth.from_mqt_np(np.concatenate([np.zeros(3), 0.9999 * axis]))
    return dataclasses.replace(base, poses=poses)


RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pg_layouts.md")


def recorded():
    """{(kind, P): (bound on |H - H_model| / max |H_model|, bound on |b - b_model| / max |b_model|)} of profiles/pg_layouts.md,
    which `python tests/test_pg_model.py` writes"""
    out = {}
    with open(RECORD) as f:
        for line in f:
            c = [x.strip() for x in line.strip().strip("|").split("|")]
            if len(c) == 8 and c[0] in KINDS:
                out[(c[0], int(c[1]))] = (float(c[6]), float(c[7]))
    return out


def recorded_scaled():
    """the same for pg_model.scaled_distance: {(kind, P): (bound on the scaled distance of H, of b)}, from the file's second
    table (six columns, so that the rows of the two tables cannot be taken for each other)"""
    out = {}
    with open(RECORD) as f:
        for line in f:
            c = [x.strip() for x in line.strip().strip("|").split("|")]
            if len(c) == 6 and c[0] in KINDS:
                out[(c[0], int(c[1]))] = (float(c[4]), float(c[5]))
    return out


def without_edges(g, drop):
    keep = np.setdiff1d(np.arange(g.O), np.asarray(drop, np.int64))
    return dataclasses.replace(g, o_i=g.o_i[keep], o_j=g.o_j[keep], o_meas=g.o_meas[keep], o_info=g.o_info[keep]), keep
