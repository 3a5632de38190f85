"""Inputs of the local-BA tests (tests/test_local_graph_model.py, tests/test_local_ba_device_gpu.py): small maps as the tables
se2gpu_local_ba_batch_device reads, the windows cut out of them, and for every rule of the gather a case that exercises it.

A map is a dict of host arrays: frame_id, Twb, Tcw, frame_null, odo_to, odo_meas, odo_cov, kps_xy (nframes, cap, 2), kps_octave,
counts, cap, view_pos, level_sigma2, pos, mp_ptr, obs_frame, obs_ftr, and the configuration K, Tbc12, huber, xrot_info, z_info.
A job is a dict(cur, local, ref, mps): the lists as se2gpu_local_window_batch_device would write them (slots / point indices)."""
import numpy as np

CAP = 16
NLEVELS = 8
K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1]], np.float32)
HUBER = float(np.float32(np.sqrt(5.991)))
XROT_INFO, Z_INFO = 1e6, 1.0
# the camera looks along the body's x axis: camera x = -body y, camera y = -body z, camera z = body x; 100 mm ahead, 300 mm up
RBC = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
TBC = np.array([100.0, 0.0, 300.0])
TBC12 = np.r_[RBC.reshape(-1), TBC]
# mvLevelSigma2 as the extractor makes it (src/ORBextractor.cpp:411-426): float products, level by level
_SCALE = np.ones(NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    _SCALE[_i] = _SCALE[_i - 1] * np.float32(1.2)
LEVEL_SIGMA2 = (_SCALE * _SCALE).astype(np.float32)


def tcw12(twb, Tbc12=TBC12):
    """rows 0-2 of Tcw = Tcb * Twb^-1 for the Se2 pose twb, as 12 floats"""
    x, y, th = (float(v) for v in twb)
    c, s = np.cos(th), np.sin(th)
    Twb = np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, 0], [0, 0, 0, 1]])
    Tbc = np.eye(4)
    Tbc[:3, :3], Tbc[:3, 3] = np.asarray(Tbc12[:9], np.float64).reshape(3, 3), Tbc12[9:]
    return (np.linalg.inv(Tbc) @ np.linalg.inv(Twb))[:3].astype(np.float32).reshape(12)


def scene(seed, nframes, m, per_point=(2, 4), spacing=300.0, pose_noise=(5.0, 0.002), point_noise=20.0, Tbc12=TBC12, K=K):
    """Key frames along a gently curved path (millimetres), points 1.5 - 4 m ahead of the key frame they were born at, each seen
    by 2-4 neighbouring key frames that still have a free feature; the tables hold the true scene plus noise, so there is
    something to optimise.  Odometry: a chain i -> i + 1 with the true relative motion.  Tbc12, K: the camera (the same random
    draws whatever it is)."""
    Tbc12, K = np.asarray(Tbc12, np.float64), np.asarray(K, np.float32)
    rng = np.random.default_rng(seed)
    truth = np.c_[spacing * np.arange(nframes) + rng.normal(0, 20, nframes), rng.normal(0, 40, nframes), rng.normal(0, 0.05, nframes)]
    Twb = (truth + np.c_[rng.normal(0, pose_noise[0], (nframes, 2)), rng.normal(0, pose_noise[1], nframes)]).astype(np.float32)
    Twb[0] = truth[0].astype(np.float32)
    Tcw = np.stack([tcw12(t, Tbc12) for t in Twb])
    Tcw_true = np.stack([tcw12(t, Tbc12) for t in truth]).astype(np.float64).reshape(nframes, 3, 4)
    kps_xy = np.zeros((nframes, CAP, 2), np.float32)
    kps_octave = np.zeros((nframes, CAP), np.int32)
    view_pos = np.tile(np.array([0, 0, 1000], np.float32), (nframes, CAP, 1))
    counts = np.zeros(nframes, np.int32)
    pos = np.zeros((m, 3), np.float32)
    lists = []
    for p in range(m):
        c = int(rng.integers(0, nframes))
        x, y, th = truth[c]
        body = np.array([rng.uniform(1500, 4000), rng.uniform(-900, 900), rng.uniform(0, 1200)])
        world = np.array([x + np.cos(th) * body[0] - np.sin(th) * body[1], y + np.sin(th) * body[0] + np.cos(th) * body[1], body[2]])
        pos[p] = (world + rng.normal(0, point_noise, 3)).astype(np.float32)
        k = int(rng.integers(per_point[0], per_point[1] + 1))
        near = sorted((f for f in range(nframes) if counts[f] < CAP and c - 2 <= f <= c + 1), key=lambda f: (abs(f - c), f))[:k]
        fr, ft = [], []
        for f in sorted(near):
            lc = Tcw_true[f, :, :3] @ world + Tcw_true[f, :, 3]
            i = int(counts[f])
            counts[f] += 1
            kps_xy[f, i] = (K[0, 0] * lc[:2] / lc[2] + K[:2, 2] + rng.normal(0, 0.5, 2)).astype(np.float32)
            kps_octave[f, i] = int(rng.integers(0, NLEVELS))
            view_pos[f, i] = (Tcw[f].reshape(3, 4)[:, :3].astype(np.float64) @ pos[p] + Tcw[f].reshape(3, 4)[:, 3]).astype(np.float32)
            fr.append(f)
            ft.append(i)
        lists.append((fr, ft))
    mp_ptr = np.zeros(m + 1, np.int32)
    mp_ptr[1:] = np.cumsum([len(f) for f, _ in lists])
    obs_frame = np.array([f for fr, _ in lists for f in fr], np.int32)
    obs_ftr = np.array([f for _, ft in lists for f in ft], np.int32)
    odo_to = np.r_[np.arange(1, nframes), -1].astype(np.int32)
    odo_meas = np.zeros((nframes, 3))
    odo_cov = np.zeros((nframes, 9))
    for i in range(nframes):
        j = min(i + 1, nframes - 1)
        c, s = np.cos(truth[i, 2]), np.sin(truth[i, 2])
        d = truth[j, :2] - truth[i, :2]
        odo_meas[i] = [c * d[0] + s * d[1], -s * d[0] + c * d[1], truth[j, 2] - truth[i, 2]]
        A = rng.normal(0, 1, (3, 3)) * np.array([3.0, 3.0, 0.002])[:, None]
        odo_cov[i] = (A @ A.T + np.diag([25.0, 25.0, 1e-5])).reshape(-1)
    return dict(frame_id=(10 + np.arange(nframes)).astype(np.int32), Twb=Twb, Tcw=Tcw, frame_null=np.zeros(nframes, np.uint8),
                odo_to=odo_to, odo_meas=odo_meas, odo_cov=odo_cov, kps_xy=kps_xy, kps_octave=kps_octave, counts=counts, cap=CAP,
                view_pos=view_pos, level_sigma2=LEVEL_SIGMA2.copy(), pos=pos, mp_ptr=mp_ptr, obs_frame=obs_frame, obs_ftr=obs_ftr,
                K=K, Tbc12=Tbc12, huber=HUBER, xrot_info=XROT_INFO, z_info=Z_INFO)


def copy_map(T):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T.items()}


def observers(T, p):
    s, e = int(T["mp_ptr"][p]), int(T["mp_ptr"][p + 1])
    return [int(f) for f in T["obs_frame"][s:e]]


def window(T, cur, local, order=None):
    """the window Map::updateLocalGraph selects for the local key frames `local` of a consistent map (no null entries): their
    points, every other observer as a reference key frame; slots by ascending frame_id, points by index"""
    nframes, m = len(T["counts"]), len(T["pos"])
    local = sorted(local, key=lambda f: int(T["frame_id"][f]))
    null = T["frame_null"]
    mps = [p for p in range(m) if any(f in local for f in observers(T, p) if 0 <= f < nframes)]
    ref = sorted({f for p in mps for f in observers(T, p) if 0 <= f < nframes and f not in local and not null[f]},
                 key=lambda f: int(T["frame_id"][f]))
    return dict(cur=cur, local=local, ref=ref, mps=mps)


def insert_entry(T, p, at, frame, ftr):
    """a copy of the map with the entry (frame, ftr) put at place `at` of point p's list"""
    T = copy_map(T)
    i = int(T["mp_ptr"][p]) + at
    T["obs_frame"] = np.insert(T["obs_frame"], i, frame).astype(np.int32)
    T["obs_ftr"] = np.insert(T["obs_ftr"], i, ftr).astype(np.int32)
    T["mp_ptr"][p + 1:] += 1
    return T


def kidnap(T, slots, seed, dxy=2000.0, dth=0.6):
    """the key frames `slots` displaced by metres and tens of degrees, as ba_cases.kidnapped does: Levenberg-Marquardt rejects
    trials from such a start.  Tcw and view_pos follow the displaced pose, as a map's would."""
    T = copy_map(T)
    rng = np.random.default_rng(seed)
    for f in slots:
        T["Twb"][f, :2] += rng.normal(0, dxy, 2).astype(np.float32)
        th = float(T["Twb"][f, 2]) + rng.normal(0, dth)
        T["Twb"][f, 2] = np.float32((th + np.pi) % (2 * np.pi) - np.pi)
        T["Tcw"][f] = tcw12(T["Twb"][f], T["Tbc12"])
    return T


# The start Levenberg-Marquardt rejects trials on: the three local key frames of the window [2, 3, 4] moved; the compiled CPU
# restatement of the solver (oracle.ba_optimize on the model's graph) takes the trials [4, 1, 1, 1, 1, 1, 1, 1, 1, 1] from it.
KIDNAP = dict(slots=[2, 3, 4], seed=2, dxy=3000.0, dth=0.8)


# ---- the cases: name -> dict(T, jobs [job], caps dict(max_local, max_ref, max_mp, max_obs, kf_list_cap, mp_list_cap), expect
# [dict per job: status and whatever the case states by hand])
CAPS = dict(max_local=6, max_ref=6, max_mp=60, max_obs=300, kf_list_cap=8, mp_list_cap=64)


def cases():
    c = {}
    base = scene(2, 10, 36)

    # no reference key frame listed: the least id (0, slot 3) is fixed, and id 1 inside the window (slot 2) is fixed too
    T = copy_map(base)
    T["frame_id"] = np.array([14, 12, 1, 0, 15, 16, 17, 18, 19, 20], np.int32)
    w = window(T, 0, [0, 1, 2, 3, 4, 5])
    w6 = dict(w, ref=[])                      # (the reference key frames are left out by hand: their observations become no edges)
    c["no_ref_least_id_and_id_1"] = dict(T=T, jobs=[w6], caps=CAPS, expect=[dict(
        status=0, local=[3, 2, 1, 0, 4, 5], fixed=[1, 1, 0, 0, 0, 0],
        odo=[(0, 4), (1, 0), (2, 1), (3, 2), (4, 5)])])   # slot -> vertex: 3 -> 0, 2 -> 1, 1 -> 2, 0 -> 3, 4 -> 4, 5 -> 5; slot 5's target 6 is outside

    # reference key frames present: they are fixed, and no local one is (ids 10..)
    w = window(base, 3, [2, 3, 4])
    c["ref_present"] = dict(T=base, jobs=[w], caps=CAPS, expect=[dict(status=0, local=[2, 3, 4], n_fixed_local=0)])

    # the odometry chain: 2 -> 3 a local member (edge), 3 -> 5 a reference member, 4 -> 7 outside the window, then a null slot, -1
    T = copy_map(base)
    w = window(T, 3, [1, 2, 3, 4])
    assert 5 in w["ref"] and 7 not in w["ref"] + w["local"]
    T["odo_to"][[1, 2, 3, 4]] = [-1, 3, 5, 7]
    c["odometry_targets"] = dict(T=T, jobs=[w], caps=CAPS, expect=[dict(status=0, odo=[(1, 2)])])   # vertices: 2 -> 1, 3 -> 2
    T2 = copy_map(T)
    T2["odo_to"][[1, 2, 3, 4]] = [2, 3, 4, 0]
    T2["frame_null"][0] = 1                   # slot 0 is null (and no member): 4 -> 0 gives no edge
    w2 = window(T2, 3, [1, 2, 3, 4])
    c["odometry_null_target"] = dict(T=T2, jobs=[w2], caps=CAPS, expect=[dict(status=0, odo=[(0, 1), (1, 2), (2, 3)])])

    # a point with no surviving edge: its only observers are outside the window (listed in mps by hand)
    w = window(base, 3, [2, 3, 4])
    lone = next(p for p in range(len(base["pos"])) if min(observers(base, p)) >= 7)
    wl = dict(w, mps=sorted(w["mps"] + [lone]))
    c["point_without_edges"] = dict(T=base, jobs=[wl], caps=CAPS, expect=[dict(status=0, empty_point=wl["mps"].index(lone))])

    # a frame listed twice in one point's list: the first entry counts
    p = w["mps"][0]
    f0 = observers(base, p)[0]
    T = insert_entry(base, p, len(observers(base, p)), f0, int(base["counts"][f0]) - 1)
    c["frame_twice"] = dict(T=T, jobs=[window(T, 3, [2, 3, 4])], caps=CAPS, expect=[dict(status=0, degree={0: len(observers(base, p))})])

    # feature indices at and past counts[f], negative, and frames out of range: none is an edge
    T = base
    for at, (fr, ft) in enumerate([(3, int(base["counts"][3])), (3, int(base["counts"][3]) + 1), (3, -1), (-1, 0), (10, 0), (3, CAP)]):
        T = insert_entry(T, p, 0, fr, ft)
    c["invalid_entries"] = dict(T=T, jobs=[window(base, 3, [2, 3, 4])], caps=CAPS,
                                expect=[dict(status=0, degree={0: len(observers(base, p))}, skipped_at_least=6)])

    # a null observer: its entries are skipped, and it is no reference key frame
    T = copy_map(base)
    wn = window(base, 3, [2, 3, 4])
    nullref = wn["ref"][0]
    T["frame_null"][nullref] = 1
    c["null_observer"] = dict(T=T, jobs=[window(T, 3, [2, 3, 4])], caps=CAPS, expect=[dict(status=0, not_ref=nullref)])

    # an octave out of range: the edge is skipped, the flag set
    T = copy_map(base)
    s = int(T["mp_ptr"][p])
    T["kps_octave"][T["obs_frame"][s], T["obs_ftr"][s]] = NLEVELS
    s2 = int(T["mp_ptr"][w["mps"][1]])
    T["kps_octave"][T["obs_frame"][s2], T["obs_ftr"][s2]] = -1
    c["octave_out_of_range"] = dict(T=T, jobs=[window(T, 3, [2, 3, 4])], caps=CAPS,
                                    expect=[dict(status=0, flags=1, degree={0: len(observers(base, p)) - 1})])

    # jobs out of range (status 1) next to one that runs
    w = window(base, 3, [2, 3, 4])
    c["job_out_of_range"] = dict(T=base, jobs=[dict(w, cur=10), w, dict(w, cur=-1), dict(w, n_local=-1)], caps=CAPS,
                                 expect=[dict(status=1), dict(status=0), dict(status=1), dict(status=1)])
    # ... and lists that name a slot or a point outside the tables (not as the window call writes them): left like a job out of range
    m = len(base["pos"])
    c["list_entry_out_of_range"] = dict(T=base, jobs=[dict(w, mps=w["mps"][:-1] + [m]), dict(w, local=[2, -1, 4]), dict(w, ref=w["ref"][:-1] + [10]), w],
                                        caps=CAPS, expect=[dict(status=1), dict(status=1), dict(status=1), dict(status=0)])

    # lists truncated by each of the four caps (status 2)
    wide = window(base, 3, [1, 2, 3, 4, 5])
    c["caps"] = dict(T=base, jobs=[wide, wide, wide, wide, wide], caps=CAPS, expect=[dict(status=2)] * 4 + [dict(status=0)],
                     job_caps=[dict(max_local=4), dict(max_ref=len(wide["ref"]) - 1), dict(max_mp=len(wide["mps"]) - 1), dict(max_obs=20), {}])
    c["list_caps"] = dict(T=base, jobs=[wide, wide, wide], caps=CAPS, expect=[dict(status=2), dict(status=2), dict(status=0)],
                          job_caps=[dict(kf_list_cap=4), dict(mp_list_cap=len(wide["mps"]) - 1), {}])

    # an odometry self loop (status 2)
    T = copy_map(base)
    T["odo_to"][3] = 3
    c["odometry_self_loop"] = dict(T=T, jobs=[window(T, 3, [2, 3, 4]), window(T, 6, [5, 6])], caps=CAPS,
                                   expect=[dict(status=2), dict(status=0)])

    # a null local key frame (status 3)
    T = copy_map(base)
    T["frame_null"][3] = 1
    c["null_local"] = dict(T=T, jobs=[dict(window(base, 3, [2, 3, 4]))], caps=CAPS, expect=[dict(status=3)])

    # every key frame fixed (status 5): one local key frame, the least id, no reference key frame listed
    w = window(base, 3, [3])
    c["all_fixed"] = dict(T=base, jobs=[dict(w, ref=[])], caps=CAPS, expect=[dict(status=5, fixed=[1])])
    # ... and a window whose points have no observer in it: no edge at all
    T = copy_map(base)
    T["odo_to"][:] = -1
    c["no_edges"] = dict(T=T, jobs=[dict(cur=3, local=[2, 3], ref=[4], mps=[lone])],
                         caps=CAPS, expect=[dict(status=5)])
    return c


def wide_landmark_case():
    """about 70 key frames; 66 reference key frames observe one point of a two-key-frame window (status 4); a second job of the
    same batch runs normally"""
    nframes = 70
    T = scene(5, nframes, 60, per_point=(2, 3))
    w = window(T, 1, [0, 1])
    p = w["mps"][0]
    have = set(observers(T, p))
    at = len(have)
    for f in range(2, 2 + 66):
        if f in have:
            continue
        i = int(T["counts"][f])
        if i >= CAP:
            i = CAP - 1                       # the feature is shared with another point: the tables allow it
        else:
            T["counts"][f] += 1
        T = insert_entry(T, p, at, f, i)
        at += 1
    w = window(T, 1, [0, 1])
    far = window(T, 68, [68, 69])
    caps = dict(max_local=4, max_ref=70, max_mp=60, max_obs=400, kf_list_cap=70, mp_list_cap=64)
    return dict(T=T, jobs=[w, far], caps=caps, expect=[dict(status=4), dict(status=0)], point=w["mps"].index(p))


def job_rows(jobs, kf_list_cap, mp_list_cap, sentinel=-9):
    """the arrays se2gpu_local_window_batch_device would have written for the jobs: job_kf, win_out (n, 4), the three lists cut at
    their caps (the counts are not)"""
    n = len(jobs)
    job_kf = np.array([j["cur"] for j in jobs], np.int32)
    out = np.zeros((n, 4), np.int32)
    ll = np.full((n, kf_list_cap), sentinel, np.int32)
    rl = np.full((n, kf_list_cap), sentinel, np.int32)
    ml = np.full((n, mp_list_cap), sentinel, np.int32)
    for i, j in enumerate(jobs):
        out[i] = [j.get("n_local", len(j["local"])), len(j["ref"]), len(j["mps"]), 0]
        for row, lst in ((ll[i], j["local"]), (rl[i], j["ref"]), (ml[i], j["mps"])):
            k = min(len(lst), len(row))
            row[:k] = lst[:k]
    return job_kf, out, ll, rl, ml
