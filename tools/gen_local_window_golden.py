"""Writes tests/golden/local_window_ref.npz: about 100 small maps built with the reference's own KeyFrame / MapPoint / Map
objects through the compiled reference's map driver (oracle/ref.py: ref_map_add_kf / add_mp / observe / covisible /
update_local_graph), and what Map::updateLocalGraph (src/Map.cpp:285-331) answered with every key frame as the current one.

    python tools/gen_local_window_golden.py

Maps of 3-12 key frames and 10-80 points; ids (mIdKF, mId) are permuted against the slots and point indices, and the
covisibility is directed (addCovisibleKF one way for some edges).  The driver builds consistent maps without nulls: both
observation sides agree, so one table serves both.  Stored: per map the ids, the points of every key frame and the
mCovisibleKFs of every key frame; per job the reference's three lists, translated from ids to slot / point indices, in the
reference's order.  Everything is uint8 but the offsets.  The coverage the tests rely on is asserted before the file is
written."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "local_window_ref.npz")
NMAPS = 100


def random_map(rng):
    nkf, m = int(rng.integers(3, 13)), int(rng.integers(10, 81))
    kf_id = rng.permutation(nkf + 4)[:nkf]                  # ids with gaps, in another order than the slots
    while np.all(np.diff(kf_id) > 0):
        kf_id = rng.permutation(nkf + 4)[:nkf]
    mp_id = rng.permutation(m + 20)[:m]
    place = rng.permutation(nkf)                            # the slot of the k-th key frame along the trajectory
    kf_obs = [[] for _ in range(nkf)]
    for p in range(m):
        c = int(rng.integers(0, nkf))
        along = {c} | {int(np.clip(c + d, 0, nkf - 1)) for d in rng.integers(-1, 2, int(rng.integers(0, 3)))}
        if rng.random() < 0.15:
            along.add(int(rng.integers(0, nkf)))            # a far observer: a reference key frame in the making
        for k in sorted(along):
            kf_obs[int(place[k])].append(p)
    adj = [[] for _ in range(nkf)]
    for k in range(nkf - 1):                                # neighbours along the trajectory, some links missing, some one-way
        a, b = int(place[k]), int(place[k + 1])
        r = rng.random()
        if r < 0.5:
            adj[a].append(b); adj[b].append(a)
        elif r < 0.65:
            adj[a].append(b)
        elif r < 0.8:
            adj[b].append(a)
    if rng.random() < 0.3:
        a, b = (int(x) for x in rng.integers(0, nkf, 2))
        if a != b and b not in adj[a]:
            adj[a].append(b)
    return kf_id, mp_id, kf_obs, adj


def main():
    from oracle import ref
    rng = np.random.default_rng(20240601)
    z = dict(kf_off=[0], mp_off=[0], kf_id=[], mp_id=[], obs_off=[0], obs=[], adj_off=[0], adj=[],
             loc_off=[0], loc=[], ref_off=[0], ref=[], mps_off=[0], mps=[])
    n_jobs = n_partial = n_with_ref = n_one_way = 0
    for _ in range(NMAPS):
        kf_id, mp_id, kf_obs, adj = random_map(rng)
        nkf, m = len(kf_id), len(mp_id)
        rm = ref.RefMap(np.eye(3), np.eye(4), 2.0)
        for a in range(nkf):
            rm.add_kf(int(kf_id[a]), a, [0.0, 0.0, 0.0], np.zeros((len(kf_obs[a]), 2)))
        for p in range(m):
            rm.add_mp(int(mp_id[p]), [0.0, 0.0, 1000.0])
        for a in range(nkf):
            for f, p in enumerate(kf_obs[a]):
                rm.observe(a, p, f)
        for a in range(nkf):
            for b in adj[a]:
                rm.covisible(a, b)
        assert not np.all(np.diff(kf_id) > 0)
        n_one_way += any(a not in adj[b] for a in range(nkf) for b in adj[a])
        slot_of = {int(i): a for a, i in enumerate(kf_id)}
        point_of = {int(i): p for p, i in enumerate(mp_id)}
        z["kf_id"] += [int(i) for i in kf_id]
        z["mp_id"] += [int(i) for i in mp_id]
        z["kf_off"].append(len(z["kf_id"]))
        z["mp_off"].append(len(z["mp_id"]))
        for a in range(nkf):
            z["obs"] += kf_obs[a]
            z["obs_off"].append(len(z["obs"]))
            z["adj"] += adj[a]
            z["adj_off"].append(len(z["adj"]))
        for cur in range(nkf):
            lk, rk, lm = rm.update_local_graph(cur)
            z["loc"] += [slot_of[int(i)] for i in lk]
            z["ref"] += [slot_of[int(i)] for i in rk]
            z["mps"] += [point_of[int(i)] for i in lm]
            for k in ("loc", "ref", "mps"):
                z[k + "_off"].append(len(z[k]))
            n_jobs += 1
            n_partial += len(lk) < nkf
            n_with_ref += len(rk) > 0
    print("jobs %d: %.0f %% select fewer key frames than the map holds, %.0f %% have a reference key frame; %d of %d maps hold "
          "a one-way edge" % (n_jobs, 100.0 * n_partial / n_jobs, 100.0 * n_with_ref / n_jobs, n_one_way, NMAPS))
    assert 2 * n_partial >= n_jobs and 2 * n_with_ref >= n_jobs and n_one_way >= 20
    arrays = {k: np.asarray(v, np.int32 if k.endswith("_off") else np.uint8) for k, v in z.items()}
    for k, v in z.items():
        assert np.array_equal(arrays[k], np.asarray(v, np.int64)), k     # nothing is cut by the uint8
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 100 * 1024


if __name__ == "__main__":
    main()
