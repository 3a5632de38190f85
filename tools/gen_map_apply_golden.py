"""tests/golden/map_apply_ref.npz: the observation lists of the reference's own map after every new key frame.

    python tools/gen_map_apply_golden.py

Feeds the reference's compiled CPU pipeline (oracle/pipeline.py, kind "cpu") with the run of tests/test_dropin_pipeline.py's
longer case - synth.frames(120), pipeline.odometry(120), cfg.fps = 10 - and records, after frame 0 and after every frame whose
record has local_ba set (new_kf reads 0 when a key frame is added and another pruned in the same frame), the key frames
(id_kf, n_obs), every key frame's (feature, map-point id) list and the map points' id, n_obs, good_prl.  Data only.

State s of the file:
    kf_ptr[s] .. kf_ptr[s + 1]     its key frames in kf_id / kf_nobs
    obs_ptr[s] .. obs_ptr[s + 1]   its (obs_kf, obs_ftr, obs_mp) triples: key frame id, feature index, map-point id
    mp_ptr[s] .. mp_ptr[s + 1]     its map points in mp_id / mp_nobs / mp_good
    frame[s]                       the frame after which it was taken
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "map_apply_ref.npz")
NFRAMES = 120


def snapshot(p):
    kfs, mps = p.keyframes(), p.mappoints()
    tri = []
    for pos, idkf in enumerate(kfs["id_kf"]):
        ftr, mp = p.observations(pos)
        tri += [(int(idkf), int(f), int(q)) for f, q in zip(ftr, mp)]
    tri = np.array(sorted(tri), np.int32).reshape(-1, 3)
    return dict(kf_id=kfs["id_kf"].astype(np.int32), kf_nobs=kfs["n_obs"].astype(np.int32), obs=tri,
                mp_id=mps["id"].astype(np.int32), mp_nobs=mps["n_obs"].astype(np.int32), mp_good=mps["good_prl"].astype(np.uint8))


def main():
    from oracle import pipeline
    from se2lam_amd import synth
    frames, odo = synth.frames(NFRAMES), pipeline.odometry(NFRAMES)
    cfg = pipeline.default_config()
    cfg.fps = 10
    states, at = [], []
    with pipeline.Pipeline("cpu", cfg) as p:
        for t in range(NFRAMES):
            r = p.feed(frames[t], odo[t])
            if t == 0 or r["local_ba"]:
                states.append(snapshot(p))
                at.append(t)
    cat = lambda k: np.concatenate([s[k] for s in states])
    ptr = lambda k: np.concatenate([[0], np.cumsum([len(s[k]) for s in states])]).astype(np.int32)
    obs = cat("obs")
    np.savez_compressed(OUT, frame=np.array(at, np.int32), kf_ptr=ptr("kf_id"), kf_id=cat("kf_id"), kf_nobs=cat("kf_nobs"),
                        obs_ptr=ptr("obs"), obs_kf=obs[:, 0].copy(), obs_ftr=obs[:, 1].copy(), obs_mp=obs[:, 2].copy(),
                        mp_ptr=ptr("mp_id"), mp_id=cat("mp_id"), mp_nobs=cat("mp_nobs"), mp_good=cat("mp_good"))
    print(OUT, os.path.getsize(OUT), "bytes,", len(states), "states")
    for s, t in zip(states, at):
        print("frame %3d: key frames %s, %d entries, %d points" % (t, list(s["kf_id"]), len(s["obs"]), len(s["mp_id"])))


if __name__ == "__main__":
    main()
