"""Inputs of the new-key-frame tests: nine key frames of a robot driving along x, map points in front of them, and the
observation lists / jobs of every named case.  Every gated quantity (depth, cosParallax, cosAngle, dist against min / max,
sinParallax) of every emitted case lies more than ten tolerances (TOL) from its threshold in the FP64 model: a world point
is redrawn until that holds, and `margins_of_*` let the CPU test assert it for the batch as a whole.
"""
import numpy as np

import new_kf_model as nk
from se2lam_amd import capi

CAP, NFRAMES = 64, 9
FX, CX, CY = 230.0, 160.0, 120.0
LOWER, UPPER = 0.3, 100.0
TOL = 5e-5            # the redraw rule's tolerance; test_new_kf_model.py asserts that the device's bound stays below it
STEP = 0.1            # metres between key frames
IDKF = np.array([0, 1, 2, 2, 4, 5, 6, 7, 8], np.int32)        # frames 2 and 3 tie
COUNTS = np.array([64, 64, 64, 64, 64, 64, 64, 63, 64], np.int32)
NEW = 8               # the frame of the observation just added
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


class Scene:
    """poses, intrinsics and an empty key-point table; add_point projects a world point into the frames of its list"""

    def __init__(self, seed=1, counts=COUNTS, idkf=IDKF, cap=CAP):
        rng = np.random.default_rng(seed)
        self.cap = cap
        K = np.array([[FX, 0, CX], [0, FX, CY], [0, 0, 1.0]])
        self.Tcw64 = []
        Tcw, Twc, P = [], [], []
        for f in range(len(idkf)):
            R = _rot_y(0.02 * rng.standard_normal())
            c = np.array([STEP * idkf[f] + (0.03 if f == 3 else 0.0), 0.01 * rng.standard_normal(), 0.02 * rng.standard_normal()])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, -R @ c
            T32 = T.astype(np.float32)                 # what the caller holds; inverse and projection derive from it
            self.Tcw64.append(T32.astype(np.float64))
            Tcw.append(T32[:3].ravel())
            Twc.append(np.linalg.inv(T32.astype(np.float64))[:3].astype(np.float32).ravel())
            P.append((K @ T32[:3].astype(np.float64)).astype(np.float32).ravel())
        self.kps = np.zeros(len(idkf) * cap, KP)
        self.kps["x"], self.kps["y"] = CX, CY
        self.kps["octave"] = 2
        self.K = K
        self.fr = nk.Frames(self.kps, counts, cap, np.array(Tcw), np.array(Twc), np.array(P), idkf)
        self.rng = rng

    def world(self, depth, f=NEW, spread=0.25):
        """a world point at `depth` in front of frame f, off the axis by up to `spread` of the depth"""
        pc = np.array([spread * depth * self.rng.uniform(-1, 1), spread * depth * self.rng.uniform(-0.6, 0.6), depth, 1.0])
        return (np.linalg.inv(self.Tcw64[f]) @ pc)[:3]

    def cam(self, f, X):
        return (self.Tcw64[f] @ np.append(X, 1.0))[:3]

    def put(self, f, k, X, octave=2, noise=0.0):
        pc = self.cam(f, X)
        uv = self.K @ (pc / pc[2])
        o = f * self.cap + k
        self.kps["x"][o], self.kps["y"][o] = uv[0] + noise * self.rng.standard_normal(), uv[1] + noise * self.rng.standard_normal()
        self.kps["octave"][o] = octave


def csr(lists):
    """lists of (frame, feature) pairs per point -> mp_ptr, obs_frame, obs_ftr"""
    return capi.csr([([e[0] for e in l], [e[1] for e in l]) for l in lists])


def _one_point(sc, entries, good=0, new=NEW):
    ptr, fr_, ft_ = csr([entries])
    mg = []
    out = nk.parallax_batch(nk.L64, sc.fr, ptr, fr_, ft_, [good], [new], FX, LOWER, UPPER, None, mg)
    return int(out["status"][0]), mg


class ParallaxCases:
    """48 points or fewer; point p uses feature p of every frame it is seen in.  names[p] says what the point is for."""

    def __init__(self, seed=1):
        self.sc = sc = Scene(seed)
        self.lists, self.good, self.new, self.names, self.want_status = [], [], [], [], []
        near, far, beyond = (2.0, 4.0), (50.0, 80.0), (130.0, 160.0)
        add = self.add
        add("promote_3", [6, 7, 8], near, 1)
        add("promote_9", [0, 1, 2, 3, 4, 5, 6, 7, 8], near, 1)
        add("promote_9_reversed", [8, 7, 6, 5, 4, 3, 2, 1, 0], near, 1)
        add("already_good", [6, 7, 8], near, 0, good=1)
        add("two_observations", [7, 8], near, 0)
        add("three_observations", [4, 7, 8], near, 1)
        add("age_6_abandoned", [2, 7, 8], far, 2)            # idkf 8 - 2 = 6: pKF0, and old enough to be abandoned
        add("age_7_excluded", [1, 7, 8], far, 3)             # idkf 8 - 1 = 7: not a candidate; pKF0 is frame 7
        add("age_5_kept", [4, 6, 8], far, 3)
        add("age_7_excluded_promoted", [1, 5, 8], near, 1)
        add("tie_first_wins_3", [3, 2, 8, 6], near, 1)       # idkf(2) == idkf(3): the first listed is pKF0, the other is skipped
        add("tie_first_wins_2", [2, 3, 8, 6], near, 1)
        add("pkf0_is_pkf", [0, 1, 8], near, 3)
        add("new_frame_absent", [5, 6, 7], near, 0, new=8)
        add("new_frame_out_of_range", [5, 6, 7], near, 0, new=NFRAMES)
        add("new_frame_negative", [5, 6, 7], near, 0, new=-1)
        add("depth_gate", [5, 7, 8], beyond, 3)
        add("depth_gate_abandoned", [3, 7, 8], beyond, 2)
        add("out_of_range_entries", [6, 7, 8], near, 1,
            extra=lambda p: [(-1, p), (6, p), (NFRAMES, p), (7, p), (5, CAP), (5, -1), (7, 63), (8, p)])
        add("out_of_range_leaves_two", [7, 8], near, 0, extra=lambda p: [(-1, p), (7, p), (NFRAMES, 0), (8, p), (7, 63)])
        add("new_at_frame_7", [2, 5, 7], near, 1, new=7)     # feature p < 63 = counts[7]
        rng = np.random.default_rng(seed + 100)
        while len(self.lists) < 48:
            n = int(rng.integers(3, 10))
            frames = sorted(rng.choice(NFRAMES - 1, n - 1, replace=False).tolist()) + [8]
            rng.shuffle(frames)
            add("random", [int(f) for f in frames], near if rng.random() < 0.7 else far, None)
        self.ptr, self.obs_frame, self.obs_ftr = csr(self.lists)
        self.good, self.new = np.array(self.good, np.uint8), np.array(self.new, np.int32)
        self.observed = np.zeros(NFRAMES * CAP, np.uint8)
        for f, k in zip(self.obs_frame, self.obs_ftr):
            if sc.fr.offset(int(f), int(k)) >= 0:
                self.observed[int(f) * CAP + int(k)] = 1

    def add(self, name, frames, depth, want, good=0, new=NEW, extra=None):
        sc, p = self.sc, len(self.lists)
        entries = [(f, p) for f in frames] if extra is None else extra(p)
        for _ in range(200):
            X = sc.world(sc.rng.uniform(*depth))
            for f in frames:
                sc.put(f, p, X, noise=0.1)
            status, mg = _one_point(sc, entries, good, new)
            if not nk.near_threshold(mg, TOL) and (want is None or status == want):
                break
        else:
            raise AssertionError("no draw of %s gives status %s with its margins" % (name, want))
        self.lists.append(entries)
        self.good.append(good)
        self.new.append(new)
        self.names.append(name)
        self.want_status.append(status)

    def run(self, L, margins=None, observed=True):
        return nk.parallax_batch(L, self.sc.fr, self.ptr, self.obs_frame, self.obs_ftr, self.good, self.new, FX, LOWER, UPPER,
                                 self.observed if observed else None, margins)

    def index(self, name):
        return self.names.index(name)


class CorrespdCases:
    """Three jobs (prev -> new) = (6 -> 8), (4 -> 7), (3 -> 5) over one scene; frames 7 and 5 hold 63 features and 1.  In job 0 feature i of prev is matched to
    feature PERM[i] of new.  ROLE[i] names what feature i of job 0's previous key frame is for."""

    JOBS = ((6, 8), (4, 7), (3, 5))

    def __init__(self, seed=2, abandoned=False):
        self.sc = sc = Scene(seed, counts=np.array([64, 64, 64, 64, 64, 1, 64, 63, 64], np.int32))
        B = len(self.JOBS)
        rng = np.random.default_rng(seed + 7)
        self.job_prev = np.array([j[0] for j in self.JOBS], np.int32)
        self.job_new = np.array([j[1] for j in self.JOBS], np.int32)
        self.matched12 = np.full((B, CAP), -1, np.int32)
        self.local_pos = np.zeros((B, CAP, 3), np.float32)
        self.match_idx_mp = np.full((B, CAP), -1, np.int32)
        self.view_pos = np.zeros((NFRAMES * CAP, 3), np.float32)
        self.observed = np.zeros(NFRAMES * CAP, np.uint8)
        self.Tcr, self.Trc = np.zeros((B, 12), np.float32), np.zeros((B, 12), np.float32)
        self.mp = dict(main_frame=[], main_ftr=[], main_octave=[], normal=[], dist=[])
        self.roles = {}
        self.tracked_lists = []          # per tracked point of job 0: its observation list with (new, j) added
        for b, (fp, fn) in enumerate(self.JOBS):
            T = sc.Tcw64[fn] @ np.linalg.inv(sc.Tcw64[fp])
            self.Tcr[b] = T[:3].astype(np.float32).ravel()
            T32 = np.eye(4)
            T32[:3] = self.Tcr[b].reshape(3, 4)
            self.Trc[b] = np.linalg.inv(T32)[:3].astype(np.float32).ravel()
            n_prev, n_new = int(sc.fr.counts[fp]), int(sc.fr.counts[fn])
            perm = rng.permutation(n_new)
            n_pairs = {0: 40, 1: 63, 2: 1}[b]        # job 1's new frame holds 63 features, job 2's holds one
            for i in range(min(n_pairs, n_prev)):
                j = int(perm[i])
                tracked = i % 3 == 0
                self._pair(b, fp, fn, i, j, tracked)
                if b == 0:
                    self.roles[i] = "tracked" if tracked else "new"
        # pass 2 of job 0: features of the new frame that no pair uses, matched to map points whose main observation is in frame 2
        free = [j for j in range(64) if j not in set(self.matched12[0].tolist())]
        kinds = ["accept", "accept", "octave", "angle", "dist_min", "dist_max", "depth", "accept", "main_out_of_range", "q_out_of_range"]
        self.pass2 = {}
        for name, j in zip(kinds, free):
            self.pass2.setdefault(name, []).append(j)
            self._map_point(name, 0, 8, j)
        self.dup = None
        if abandoned:
            self._abandon()
        for k in ("main_frame", "main_ftr", "main_octave"):
            self.mp[k] = np.array(self.mp[k], np.int32)
        self.mp["normal"] = np.array(self.mp["normal"], np.float32).reshape(-1, 3)
        self.mp["dist"] = np.array(self.mp["dist"], np.float32).reshape(-1, 2)

    def _pair(self, b, fp, fn, i, j, tracked):
        sc = self.sc
        for _ in range(200):
            X = sc.world(sc.rng.uniform(2.0, 5.0), fn)
            sc.put(fp, i, X, noise=0.3)
            sc.put(fn, j, X, noise=0.3)
            self.matched12[b, i] = j
            pc = sc.cam(fp, X) * (1 + 0.01 * sc.rng.standard_normal())
            if tracked:
                self.view_pos[fp * CAP + i] = pc
                self.observed[fp * CAP + i] = 1
                mg = []
                nk.L64.se3_to_xyz_info(self.view_pos[fp * CAP + i], nk.EYE12, self.Tcr[b], self.Trc[b], FX, mg)
            else:
                self.local_pos[b, i] = pc
                mg = []
                nk.L64.se3_to_xyz_info(self.local_pos[b, i], sc.fr.Twc[fp], sc.fr.Tcw[fn], sc.fr.Twc[fn], FX, mg)
            if not nk.near_threshold(mg, TOL):
                return
        raise AssertionError("no draw")

    def _map_point(self, name, b, fn, j, main=(2, None)):
        """a map point whose main observation is feature 40 + q of frame 2, matched to feature j of the new frame"""
        sc, q = self.sc, len(self.mp["main_frame"])
        fm, km = main[0], 40 + q
        depth = (130.0, 160.0) if name == "depth" else (2.0, 5.0)
        for _ in range(200):
            X = sc.world(sc.rng.uniform(*depth), fn)
            sc.put(fm, km, X, noise=0.2)
            sc.put(fn, j, X, octave=5 if name == "octave" else 2, noise=0.2)
            pc = sc.cam(fn, X)
            d = np.linalg.norm(pc)
            normal = pc / d
            if name == "angle":
                normal = _rot_y(np.deg2rad(40.0)) @ normal
            lo, hi = {"dist_min": (1.2 * d, 2 * d), "dist_max": (0.3 * d, 0.8 * d)}.get(name, (0.6 * d, 1.6 * d))
            row = dict(main_frame=fm, main_ftr=km, main_octave=2, normal=normal.astype(np.float32), dist=np.array([lo, hi], np.float32))
            if name == "main_out_of_range":
                row["main_ftr"] = CAP
            mg = []
            x3d = nk.L64.triangulate(sc.fr.pt(fm * CAP + km), sc.fr.pt(fn * CAP + j), sc.fr.P[fm], sc.fr.P[fn])
            pos = nk.L64.se3map(sc.fr.Tcw[fn], x3d)
            acc = nk.accept_new_observe(nk.L64, pos, row["normal"], 2, sc.kps["octave"][fn * CAP + j], lo, hi, mg)
            dep = nk._depth_ok(nk.L64, pos[2], LOWER, UPPER, mg)
            if acc and dep:
                nk.L64.se3_to_xyz_info(pos, sc.fr.Twc[fn], sc.fr.Tcw[fm], sc.fr.Twc[fm], FX, mg)
            fails = [n for n, v, t in mg if (n == "cosAngle" and v < t) or (n == "dist_min" and v < t) or (n == "dist_max" and v > t)
                     or (n == "depth_lower" and v < t) or (n == "depth_upper" and v > t)]
            alone = {"angle": ["cosAngle"], "dist_min": ["dist_min"], "dist_max": ["dist_max"], "depth": ["depth_upper"]}.get(name, [])
            if not nk.near_threshold(mg, TOL) and fails == alone:
                break
        else:
            raise AssertionError("no draw of map point %s" % name)
        for k in self.mp:
            self.mp[k].append(row[k])
        self.match_idx_mp[b, j] = 999 if name == "q_out_of_range" else q
        return q

    def _abandon(self):
        """tracked pair 0 of job 0 becomes a far point seen from frames 2 and 6: after pass 1 adds (8, j) its parallax update
        abandons it, and a map point matched to the freed feature j is there for pass 2"""
        sc, b, fp, fn, i = self.sc, 0, 6, 8, 0
        j = int(self.matched12[b, i])
        for _ in range(200):
            X = sc.world(sc.rng.uniform(50.0, 80.0), fn)
            for f, k in ((2, 39), (fp, i), (fn, j)):
                sc.put(f, k, X, noise=0.2)
            self.view_pos[fp * CAP + i] = sc.cam(fp, X)
            entries = [(2, 39), (fp, i), (fn, j)]
            status, mg = _one_point(sc, entries, 0, fn)
            nk.L64.se3_to_xyz_info(self.view_pos[fp * CAP + i], nk.EYE12, self.Tcr[b], self.Trc[b], FX, mg)
            if status == 2 and not nk.near_threshold(mg, TOL):
                break
        else:
            raise AssertionError("no draw of the abandoned point")
        self.observed[2 * CAP + 39] = 1
        self.abandoned = dict(entries=entries, i=i, j=j)
        # the map point for the freed feature: main observation in frame 3, at a usual depth, consistent with feature j of frame 8
        q = len(self.mp["main_frame"])
        for _ in range(200):
            Xn = sc.world(sc.rng.uniform(2.0, 5.0), fn)
            pc = sc.cam(fn, Xn)
            # move the world point onto the ray of feature j as it stands, so the far point's projection in frame 8 stays
            ray = np.linalg.inv(sc.K) @ np.array([sc.kps["x"][fn * CAP + j], sc.kps["y"][fn * CAP + j], 1.0])
            Xn = (np.linalg.inv(sc.Tcw64[fn]) @ np.append(ray * pc[2], 1.0))[:3]
            sc.put(3, 40 + q, Xn, noise=0.0)
            pc = sc.cam(fn, Xn)
            d = np.linalg.norm(pc)
            row = dict(main_frame=3, main_ftr=40 + q, main_octave=2, normal=(pc / d).astype(np.float32),
                       dist=np.array([0.6 * d, 1.6 * d], np.float32))
            mg = []
            x3d = nk.L64.triangulate(sc.fr.pt(3 * CAP + 40 + q), sc.fr.pt(fn * CAP + j), sc.fr.P[3], sc.fr.P[fn])
            pos = nk.L64.se3map(sc.fr.Tcw[fn], x3d)
            ok = nk.accept_new_observe(nk.L64, pos, row["normal"], 2, 2, row["dist"][0], row["dist"][1], mg) and \
                nk._depth_ok(nk.L64, pos[2], LOWER, UPPER, mg)
            if ok:
                nk.L64.se3_to_xyz_info(pos, sc.fr.Twc[fn], sc.fr.Tcw[3], sc.fr.Twc[3], FX, mg)
            if ok and not nk.near_threshold(mg, TOL):
                break
        else:
            raise AssertionError("no draw of the map point behind the abandoned one")
        for k in self.mp:
            self.mp[k].append(row[k])
        self.abandoned["q"] = q

    def run(self, L, passes, observed=None, match_idx_mp="own", margins=None, jobs=None):
        sel = list(range(len(self.JOBS))) if jobs is None else list(jobs)
        mi = self.match_idx_mp if isinstance(match_idx_mp, str) else match_idx_mp
        return nk.correspd_batch(L, self.sc.fr, self.observed if observed is None else observed, self.view_pos,
                                 self.job_prev[sel], self.job_new[sel], self.Tcr[sel], self.Trc[sel], self.matched12[sel],
                                 self.local_pos[sel], None if mi is None else mi[sel], self.mp, FX, LOWER, UPPER, passes, margins)


def restatement_errors(pc, cc_list):
    """worst relative error of the float32 restatement against the FP64 layer: (positions, informations); the integer
    outputs must agree exactly"""
    ep, em = [], []
    a, b = pc.run(nk.L64), pc.run(nk.L32)
    for k in ("status", "place", "kf_observed"):
        assert np.array_equal(a[k], b[k]), k
    w = a["status"] == 1
    ep.append(nk.rel_err_pos(b["pos"][w], a["pos"][w]))
    w = a["obs_view"][:, 0] != nk.SENT
    assert np.array_equal(w, b["obs_view"][:, 0] != nk.SENT)
    ep.append(nk.rel_err_pos(b["obs_view"][w], a["obs_view"][w]))
    em.append(nk.rel_err_mat(b["obs_info"][w], a["obs_info"][w]))
    for cc in cc_list:
        for passes in (7, 1, 6):
            a, b = cc.run(nk.L64, passes), cc.run(nk.L32, passes)
            for k in ("inv", "kind", "src", "counts", "kf_observed"):
                assert np.array_equal(a[k], b[k]), k
            w, w3 = a["kind"] > 0, a["kind"] == 3
            ep += [nk.rel_err_pos(b["view"][w], a["view"][w]), nk.rel_err_pos(b["new_pos_w"][w3], a["new_pos_w"][w3])]
            em += [nk.rel_err_mat(b["info"][w], a["info"][w]), nk.rel_err_mat(b["info_prev"][w3], a["info_prev"][w3])]
    return float(np.concatenate(ep).max()), float(np.concatenate(em).max())


# ---- the header's host functions (include/se2lam_amd/FindCorrespd.h) through tests/cpp_find_correspd.cpp

def cpp_build(outdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(str(outdir), "cpp_find_correspd")
    libdir = os.path.join(root, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_find_correspd.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()


def cpp_run_parallax(program, path, fr, ptr, obs_frame, obs_ftr, good, new, observed, fx=FX, lower=LOWER, upper=UPPER, lines=()):
    """updateParallax for every point of the CSR, after the "I" lines given.  Returns their output rows and the outputs of
    nk.parallax_batch as float32."""
    import subprocess
    m, nobs = len(ptr) - 1, len(obs_frame)
    head = [fr.nframes, fr.cap, m, nobs] + list(fr.counts) + list(fr.idkf) + bits(fr.Tcw) + bits(fr.Twc) + bits(fr.P) + \
        bits(fr.kps["x"]) + bits(fr.kps["y"]) + list(ptr) + list(obs_frame) + list(obs_ftr) + list(good) + list(new) + \
        bits([fx, lower, upper]) + list(observed)
    with open(str(path), "w") as f:
        f.write("\n".join(list(lines) + ["P " + " ".join(str(int(v)) for v in head)]) + "\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = r.stdout.splitlines()
    n = len(lines)
    pts = np.array([[int(x) for x in ln.split()] for ln in rows[n:n + m]], np.int64).reshape(m, 5)
    ob = np.array([[int(x) for x in ln.split()] for ln in rows[n + m:n + m + nobs]], np.int64).reshape(nobs, 12)
    ob = ob.astype(np.uint32).view(np.float32)
    return rows[:n], dict(status=pts[:, 0].astype(np.int32), place=pts[:, 1].astype(np.int32),
                          pos=pts[:, 2:5].astype(np.uint32).view(np.float32), obs_view=ob[:, :3], obs_info=ob[:, 3:],
                          kf_observed=np.array([int(x) for x in rows[n + m + nobs].split()], np.uint8))


def same_parallax(got, ref):
    """the host mirror against the float32 restatement: integers exactly, the DLT to the bit (no library call in it), the
    rest to 4e-6 relative - the two sides differ in asinf / sin / cos of the C library against numpy's alone"""
    nobs = len(got["obs_view"])
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["place"], ref["place"])
    assert np.array_equal(got["pos"].view(np.uint32), ref["pos"].view(np.uint32))
    w = ref["obs_view"][:nobs, 0] != nk.SENT
    assert np.array_equal(got["obs_view"][:, 0] != np.float32(nk.SENT), w)
    assert w.any()
    assert nk.rel_err_pos(got["obs_view"][w], ref["obs_view"][:nobs][w]).max() < 4e-6
    assert nk.rel_err_mat(got["obs_info"][w], ref["obs_info"][:nobs][w]).max() < 4e-6
    assert np.array_equal(got["kf_observed"], ref["kf_observed"])
