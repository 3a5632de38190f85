"""tests/golden/map_apply_ref.npz (tools/gen_map_apply_golden.py) as cases of tests/map_apply_model.py: the states of the
reference's map after every new key frame, and the job rows that lead from one to the next.
Key frame id k lives in frame slot k - 1; map point slots are the ranks of MapPoint::mId, the order the reference created them in."""
import os

import numpy as np

import map_apply_model as mm

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_apply_ref.npz")
f32 = np.float32


class Golden:
    def __init__(self):
        g = np.load(PATH)
        self.states = []
        for s in range(len(g["frame"])):
            k, o, m = (slice(g[n][s], g[n][s + 1]) for n in ("kf_ptr", "obs_ptr", "mp_ptr"))
            self.states.append(dict(kf_id=g["kf_id"][k], kf_nobs=g["kf_nobs"][k], obs_kf=g["obs_kf"][o], obs_ftr=g["obs_ftr"][o],
                                    obs_mp=g["obs_mp"][o], mp_id=g["mp_id"][m], mp_nobs=g["mp_nobs"][m], mp_good=g["mp_good"][m]))
        ids, seen = np.unique(np.concatenate([st["mp_id"] for st in self.states])), 0
        for st in self.states:                               # mId grows with every point created; a point left without
            fresh = st["mp_id"][st["mp_id"] > (ids[seen - 1] if seen else -1)]   # observations leaves the map (MapPoint::setNull)
            assert np.array_equal(np.sort(fresh), ids[seen:seen + len(fresh)]) and np.isin(st["mp_id"], ids[:seen + len(fresh)]).all()
            seen += len(fresh)
            st["m"] = seen                                   # slots handed out so far
        self.slot_of = {int(i): n for n, i in enumerate(ids)}
        self.nframes = int(max(st["kf_id"].max() for st in self.states))
        self.cap = int(max(st["obs_ftr"].max() for st in self.states if len(st["obs_ftr"]))) + 1
        self.m_cap = len(ids) + 22
        self.nobs_cap = int(max(len(st["obs_kf"]) for st in self.states)) + 1100
        self.transitions = []
        for s in range(len(self.states) - 1):
            a, b = self.states[s], self.states[s + 1]
            new = [int(k) for k in b["kf_id"] if k not in a["kf_id"]]
            gone = [int(k) for k in a["kf_id"] if k not in b["kf_id"]]
            assert len(new) == 1 and len(gone) <= 1
            prev = int(a["kf_id"].max())                     # Map::getCurrentKF()
            assert new[0] > prev and prev not in gone
            of_new = b["obs_kf"] == new[0]
            old_ids = set(a["mp_id"].tolist())
            created = sorted(set(b["mp_id"].tolist()) - old_ids)
            self.transitions.append(dict(index=s, state=b, prev=prev - 1, new=new[0] - 1, pruned=gone[0] - 1 if gone else None,
                                         n_new_entries=int(of_new.sum()), n_created=len(created)))
        self.ntransitions = len(self.transitions)

    def view(self, f, k):
        return np.array([0.37 * k - 150.0 + f, 90.0 - 0.21 * k, 2900.0 + 3.0 * f + 0.01 * k], f32)

    def first_case(self):
        st = self.states[0]
        assert len(st["obs_kf"]) == 0 and len(st["mp_id"]) == 0
        return mm.blank_case(self.cap, self.nframes, self.m_cap, self.nobs_cap)

    def add_case(self, c, t):
        """the rows of the new key frame: entries on old points become kind 1 (the previous key frame holds the point) or 2,
        entries on new points kind 3 with src = the previous key frame's feature"""
        st, cap = t["state"], self.cap
        c = mm.set_jobs(dict(c), [(t["prev"], t["new"])])
        m_old = int(c["sizes_in"][0])
        held = {int(p): i for i, p in enumerate(c["ftr_mp"][t["prev"] * cap:(t["prev"] + 1) * cap]) if p >= 0}
        prev_ftr = {int(mp): int(k) for f, k, mp in zip(st["obs_kf"], st["obs_ftr"], st["obs_mp"]) if f - 1 == t["prev"]}
        good = dict(zip(st["mp_id"].tolist(), st["mp_good"].tolist()))
        for f, j, mp in zip(st["obs_kf"], st["obs_ftr"], st["obs_mp"]):
            if f - 1 != t["new"]:
                continue
            j, p = int(j), self.slot_of[int(mp)]
            if p < m_old:
                c["kind"][0, j], c["src"][0, j] = (1, held[p]) if p in held else (2, p)
            else:
                i = prev_ftr[int(mp)]
                c["kind"][0, j], c["src"][0, j] = 3, i
                c["local_pos"][0, i] = self.view(t["prev"], i)
                c["new_pos_w"][0, j] = self.view(t["new"], j) + f32(5)
                c["info_prev"][0, j] = np.arange(9, dtype=f32) + f32(i)
                c["good_prl_row"][0, i] = good[int(mp)]
            c["view"][0, j] = self.view(t["new"], j)
            c["info"][0, j] = np.arange(9, dtype=f32) * f32(2) + f32(j)
        return c

    def erase_case(self, c, out, t):
        """B = 0 with the pruned key frame null (it stays null from then on)"""
        d = mm.next_case(c, out)
        if t["pruned"] is not None:
            d["frame_null"][t["pruned"]] = 1
        return d

    def check_state(self, out, t):
        st = t["state"]
        m = int(out["sizes_out"][mm.M_NEW])
        assert m == st["m"]
        alive = np.zeros(m, bool)
        alive[[self.slot_of[int(i)] for i in st["mp_id"]]] = True
        assert np.array_equal(out["mp_null"][:m] == 0, alive)                         # which points exist
        got = mm.lists_of(out["mp_ptr_new"], out["obs_frame_new"], out["obs_ftr_new"], m)
        want = [set() for _ in range(m)]
        for f, k, mp in zip(st["obs_kf"], st["obs_ftr"], st["obs_mp"]):
            want[self.slot_of[int(mp)]].add((int(f) - 1, int(k)))
        nobs = dict(zip(st["mp_id"].tolist(), st["mp_nobs"].tolist()))
        for mp, p in self.slot_of.items():
            if p < m:
                assert set(got[p]) == want[p] and len(got[p]) == len(want[p]) == nobs.get(mp, 0), (t["index"], p)   # the entry set, n_obs
        per_frame = np.bincount(out["obs_frame_new"][:out["sizes_out"][mm.NOBS_NEW]], minlength=self.nframes)
        for k, n in zip(st["kf_id"], st["kf_nobs"]):
            assert per_frame[k - 1] == n, (t["index"], k)                             # KeyFrame::getSizeObsMP
        assert per_frame.sum() == st["kf_nobs"].sum()                                 # and nothing of a pruned key frame
        held = out["ftr_mp"] >= 0
        assert held.sum() == per_frame.sum() and np.array_equal(out["kf_observed"] != 0, held)
