"""Writes tests/golden/local_graph_ref.npz: small maps built with the reference's own KeyFrame / MapPoint / Map objects through
the compiled reference's map driver (oracle/ref.py), and the graph Map::loadLocalGraph (src/Map.cpp:891-1053) put into the
recording optimizer for one window of each.

    python tools/gen_local_graph_golden.py

The maps are those of tests/local_ba_cases.scene (6-12 key frames, 20-40 points, 16 features per key frame at most) with the
KeyFrame::id permuted, the id 1 present in some, windows with and without reference key frames, and the odometry chain cut in
places.  The driver builds consistent maps without nulls.  Stored per map: the tables the device call reads (Tcw is the
reference's own float Tcw), the window's three lists as slots / point indices in the reference's order, and the reference's
vertices, PreSE2 edges and EdgeSE2XYZ edges.  tests/test_local_graph_model.py holds the numpy model to it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "local_graph_ref.npz")
NMAPS = 24
TABLES = ("frame_id", "Twb", "Tcw", "odo_to", "odo_meas", "odo_cov", "kps_xy", "kps_octave", "counts", "view_pos", "level_sigma2", "pos",
          "mp_ptr", "obs_frame", "obs_ftr", "K", "Tbc12")


def main():
    import local_ba_cases as lc
    from oracle import ref
    rng = np.random.default_rng(20240915)
    z = {}
    with_ref = without_ref = with_id1 = 0
    for i in range(NMAPS):
        nframes, m = int(rng.integers(6, 13)), int(rng.integers(20, 41))
        T = lc.scene(1000 + i, nframes, m)
        ids = (rng.permutation(nframes + 5)[:nframes] + (2 if i % 3 else 0)).astype(np.int32)   # every third map may hold the ids 0 and 1
        T["frame_id"] = ids
        T["odo_to"][rng.random(nframes) < 0.2] = -1
        if i % 4 == 0:
            a = int(rng.integers(0, nframes - 2))
            T["odo_to"][a] = a + 2                               # not the next key frame
        bTc = np.eye(4)
        bTc[:3, :3], bTc[:3, 3] = lc.RBC, lc.TBC
        mref = ref.RefMap(T["K"], bTc, np.float32(T["huber"]), T["xrot_info"], 1e6, T["z_info"], lc.NLEVELS, 1.2)
        for a in range(nframes):
            n = int(T["counts"][a])
            mref.add_kf(100 + int(ids[a]), int(ids[a]), T["Twb"][a], T["kps_xy"][a, :n], T["kps_octave"][a, :n], T["view_pos"][a, :n])
        for p in range(m):
            mref.add_mp(1000 + p, T["pos"][p])
        for p in range(m):
            for e in range(int(T["mp_ptr"][p]), int(T["mp_ptr"][p + 1])):
                mref.observe(int(T["obs_frame"][e]), p, int(T["obs_ftr"][e]))
        for a in range(nframes):
            if T["odo_to"][a] >= 0:
                mref.set_odo(a, int(T["odo_to"][a]), T["odo_meas"][a], T["odo_cov"][a].reshape(3, 3))
        cur = int(rng.integers(0, nframes))
        local = list(range(nframes)) if i % 5 == 0 else [f for f in range(nframes) if abs(f - cur) <= int(rng.integers(0, 3))]
        for f in local:
            if f != cur:
                mref.covisible(cur, f)
                mref.covisible(f, cur)
        T["Tcw"] = np.stack([mref.kf_pose(a)[:3].reshape(12) for a in range(nframes)]).astype(np.float32)
        lk, rk, lm = mref.update_local_graph(cur)
        slot_of = {100 + int(ids[a]): a for a in range(nframes)}
        lk, rk, lm = [slot_of[int(x)] for x in lk], [slot_of[int(x)] for x in rk], [int(x) - 1000 for x in lm]
        assert sorted(lk) == sorted(local)
        out = mref.load_local_graph()
        P = len(lk) + len(rk)
        assert out["v_id"].tolist() == list(range(P)) + [P + 1 + k for k in range(len(lm))]
        for k in TABLES:
            z["m%d_%s" % (i, k)] = np.asarray(T[k])
        z["m%d_cfg" % i] = np.array([T["huber"], T["xrot_info"], T["z_info"], cur], np.float64)
        z["m%d_local" % i], z["m%d_ref" % i], z["m%d_mps" % i] = (np.array(x, np.int32) for x in (lk, rk, lm))
        z["m%d_v_est" % i], z["m%d_v_fixed" % i] = out["v_est"], out["v_fixed"].astype(np.uint8)
        z["m%d_o_ids" % i], z["m%d_o_meas" % i], z["m%d_o_info" % i] = out["o_ids"], out["o_meas"], out["o_info"]
        e_ids = out["e_ids"].copy()
        e_ids[:, 1] -= P + 1                                     # landmark index
        z["m%d_e_ids" % i], z["m%d_e_uv" % i], z["m%d_e_info" % i] = e_ids, out["e_uv"], out["e_info"]
        with_ref += bool(rk)
        without_ref += not rk
        with_id1 += bool(out["v_fixed"][:len(lk)].any() and rk)
    assert with_ref >= 8 and without_ref >= 3 and with_id1 >= 1, (with_ref, without_ref, with_id1)
    z["nmaps"] = np.array([NMAPS], np.int32)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes;", with_ref, "windows with reference key frames,", without_ref, "without,", with_id1,
          "with the id 1 fixed next to reference key frames")


if __name__ == "__main__":
    main()
