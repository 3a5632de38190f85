"""Small maps as flat tables for se2gpu_localizer_ba_batch_device, its numpy model and the CPU checks on them: the geometry of
_case in tests/test_pose_ba.py (camera over a plane, points 1.5 - 8 m ahead, 0.7 px noise, 10 % outliers of up to 50 px, starts
40 mm / 0.03 rad off), nframes = 6 frames of cap = 320 features over m = 400 points.  Positions, key points and Tcw are rounded
to float, as the tables hold them."""
import numpy as np

from test_pose_ba import CX, CY, DELTA, F, TBC, _Twb

NFRAMES, CAP, M, NLEVELS = 6, 320, 400, 8
EDGES = (0, 6, 37, 257, 300, 31)          # edges of frame f: none; few; a wave partly empty; more than one edge on a thread; most of
                                          # the row; one more than the gate's 30
N_NULL, N_BAD = 5, 5                      # the last points of the table: null, then without good parallax
GOOD = M - N_NULL - N_BAD


def inv_level_sigma2():
    """mvInvLevelSigma2 as ORBextractor fills it: float products of the scale factor 1.2f"""
    sf = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        sf[i] = sf[i - 1] * np.float32(1.2)
    return (np.float32(1.0) / (sf * sf)).astype(np.float32)


def tbc12(Tbc=TBC):
    return np.concatenate([Tbc[:3, :3].reshape(-1), Tbc[:3, 3]]).astype(np.float64)


def tables(seed=0, edges=EDGES, shift_uv=None, Tbc=TBC, cam=(F, CX, CY)):
    """shift_uv = (frame, pixels): every key point of that frame moved, so that every edge is a gross outlier and LM rejects trials.
    Tbc (4x4), cam = (f, cx, cy): the camera; the random draws are the same whatever it is."""
    TBC, (F, CX, CY) = np.asarray(Tbc, np.float64), cam
    rng = np.random.default_rng(seed)
    pose = np.array([rng.uniform(-2000, 2000), rng.uniform(-2000, 2000), rng.uniform(-3, 3)])
    Twc_ref = _Twb(*pose) @ TBC
    Xc = np.stack([rng.uniform(-2000, 2000, M), rng.uniform(-1500, 1500, M), rng.uniform(1500, 8000, M)], 1)
    pos = (Twc_ref @ np.c_[Xc, np.ones(M)].T).T[:, :3].astype(np.float32)
    mp_null, good_prl = np.zeros(M, np.uint8), np.ones(M, np.uint8)
    mp_null[GOOD:GOOD + N_NULL] = 1
    good_prl[GOOD + N_NULL:] = 0
    T = dict(Tcw=np.zeros((NFRAMES, 12), np.float32), Twb=np.zeros((NFRAMES, 3), np.float32), kps_xy=np.zeros((NFRAMES, CAP, 2), np.float32),
             kps_octave=np.zeros((NFRAMES, CAP), np.int32), counts=np.zeros(NFRAMES, np.int32), ftr_mp=np.full((NFRAMES, CAP), -1, np.int32),
             kf_observed=np.zeros((NFRAMES, CAP), np.uint8), pos=pos, mp_null=mp_null, good_prl=good_prl, inv_level_sigma2=inv_level_sigma2(),
             Tbc12=tbc12(TBC), xrot_info=1e6, yrot_info=1e6, z_info=1.0, K=np.array([[F, 0, CX], [0, F, CY], [0, 0, 1]], np.float32),
             huber=DELTA, true_pose=np.zeros((NFRAMES, 3)), plan=[])
    for f in range(NFRAMES):
        true = pose + np.r_[rng.normal(0, 60, 2), rng.normal(0, 0.02)]            # every frame looks at the same part of the map
        Tcw_true = np.linalg.inv(_Twb(*true) @ TBC)
        start = true + np.r_[rng.normal(0, 40, 2), rng.normal(0, 0.03)]
        Tcw0 = np.linalg.inv(_Twb(*start) @ TBC)
        T["true_pose"][f] = true
        T["Tcw"][f] = Tcw0[:3, :4].reshape(12)
        T["Twb"][f] = start
        E = edges[f]
        extra = 4 if E else 0                                                     # two null and two bad-parallax observations
        n = min(CAP - 1, E + extra + 15)                                          # (319 for the fullest row: not a multiple of anything)
        T["counts"][f] = n
        pts = np.concatenate([rng.choice(GOOD, E, replace=False), [GOOD, GOOD + 1, GOOD + N_NULL, GOOD + N_NULL + 1][:extra]]).astype(np.int64)
        ftrs = rng.choice(n, len(pts), replace=False)
        T["ftr_mp"][f, ftrs] = pts
        T["kf_observed"][f, ftrs] = 1
        T["kps_octave"][f] = rng.integers(0, NLEVELS, CAP)
        T["kps_xy"][f] = rng.uniform(0, 640, (CAP, 2))
        Xf = (Tcw_true @ np.c_[pos[pts].astype(np.float64), np.ones(len(pts))].T).T[:, :3]
        uv = F * Xf[:, :2] / Xf[:, 2:] + [CX, CY] + rng.normal(0, 0.7, (len(pts), 2))
        out = rng.random(len(pts)) < 0.1
        uv[out] += rng.uniform(-50, 50, (int(out.sum()), 2))
        T["kps_xy"][f, ftrs] = uv
        # what a match row can renew (match_rows): free features that show points the frame does not hold yet, a free feature
        # behind the frame's first observation that shows that observation's point, a free feature before its last one
        free = np.setdiff1d(np.arange(n), ftrs)
        rng.shuffle(free)
        plan = dict(new=(free[:0], free[:0]), move=None, stay=None, change=None, spare=free)
        if E:
            unseen = rng.permutation(np.setdiff1d(np.arange(GOOD), pts))
            held = np.sort(ftrs[:E])
            lo, hi = int(held[0]), int(held[-1])
            plan["new"] = (free[:4], unseen[:4])
            rest = free[4:]
            later, earlier = rest[rest > lo], rest[rest < hi]
            if len(later):
                plan["move"] = (int(later[0]), int(T["ftr_mp"][f, lo]))
            earlier = earlier[earlier != (later[0] if len(later) else -1)]
            if len(earlier):
                plan["stay"] = (int(earlier[0]), int(T["ftr_mp"][f, hi]))
            if E >= 30:                                                           # one more outlier: the feature shows its old point
                plan["change"] = (int(held[E // 2]), int(unseen[4]))
            used = [plan[k][0] for k in ("move", "stay") if plan[k]]
            plan["spare"] = np.setdiff1d(rest, used)
            shown = [(j, q) for j, q in zip(*plan["new"])] + ([plan["move"]] if plan["move"] else [])
            for j, q in shown:
                X = Tcw_true @ np.r_[pos[q].astype(np.float64), 1.0]
                T["kps_xy"][f, j] = F * X[:2] / X[2] + [CX, CY] + rng.normal(0, 0.7, 2)
        T["plan"].append(plan)
        # features past counts hold plausible entries that must not be read
        T["ftr_mp"][f, n:] = rng.integers(0, GOOD, CAP - n)
    if shift_uv is not None:
        T["kps_xy"][shift_uv[0]] += np.float32(shift_uv[1])
    return T


def match_rows(T, frames, seed=1):
    """Rows as se2gpu_match_projection_device writes them, one per job, that exercise the renewal by the frame's plan: free features
    matched to points the frame does not hold, a point that moves to a greater feature, a point that stays with the greater feature
    (the lower is dropped), an observed feature that changes its point, a null point, and indices that name no point."""
    rng = np.random.default_rng(seed)
    rows = np.full((len(frames), CAP), -1, np.int32)
    for b, f in enumerate(frames):
        if not 0 <= f < NFRAMES:
            continue
        n, plan = int(T["counts"][f]), T["plan"][f]
        rows[b, plan["new"][0]] = plan["new"][1]
        for k in ("move", "stay", "change"):
            if plan[k]:
                rows[b, plan[k][0]] = plan[k][1]
        spare = plan["spare"]
        rows[b, spare[0]] = GOOD + 2                                               # a null point: addObservation returns
        rows[b, spare[1]], rows[b, spare[2]] = M + 5, -3                           # no point
        rows[b, n:] = rng.integers(0, GOOD, CAP - n)                               # past counts: never read
    return rows


HISTORY_FRAMES = (1, 2, 3, 4, 5)          # the frames of tables() whose LM histories the GPU test compares (frame 0 has no edge)
REJECT = (2, 400.0)                       # tables(shift_uv=REJECT): frame 2 with every edge an outlier


def live_iterations(stats):
    """the leading iterations of an LM history whose cost drops by at least 1e-9 relative: what _same_run of tests/test_pose_ba.py
    compares trial by trial"""
    h = np.asarray(stats["chi2_hist"])
    prev = np.concatenate([[stats["chi2_init"]], h[:-1]])
    dead = (prev - h) < 1e-9 * h
    return int(np.argmax(dead)) if dead.any() else len(h)


def matrix(p12):
    T = np.eye(4)
    T[:3, :3] = np.asarray(p12[:9]).reshape(3, 3)
    T[:3, 3] = p12[9:12]
    return T
