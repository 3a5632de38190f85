"""The scenes and batches that the tests of se2gpu_track_frames_batch_device share (tests/test_track_frame_model.py asserts on
the CPU that every case has the property it is there for, tests/test_track_frames_device_gpu.py runs them on the device).

Scene: frames 2k and 2k+1 hold the two views of a seeded set of points in front of a camera that turns a little about y and
moves by a baseline of its own (millimetres), each view in a random feature order of its own, the rest of the row up to cap
filled with further points (counts decides what is a feature).  Depths run from 300 to 12,000 mm, so the gate 500..8000 rejects
some, and with baselines of 40..300 mm the two-degree parallax test passes for the near points and fails for the far ones.  A
share of the second view is moved by up to 80 px: the outliers of the epipolar filter."""
import numpy as np

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])
K = np.array([[400.0, 0, 320.0], [0, 400.0, 240.0], [0, 0, 1]], np.float32)
P_REF = (K @ np.eye(3, 4, dtype=np.float32)).astype(np.float32).reshape(-1)      # Config::PrjMtrxEye
LOWER, UPPER, MIN_DEGREE = 500.0, 8000.0, 2
SENTINEL = 7


class Scene:
    def __init__(self, cap, n_points, outliers, baselines, seed=2025):
        rng = np.random.default_rng(seed)
        self.cap, self.nframes = cap, 2 * len(n_points)
        self.kps = np.zeros((self.nframes, cap), KP)
        self.kps["x"] = rng.uniform(0, 640, (self.nframes, cap)).astype(np.float32)
        self.kps["y"] = rng.uniform(0, 480, (self.nframes, cap)).astype(np.float32)
        self.counts = np.zeros(self.nframes, np.int32)
        self.where, self.Tcr = [], []
        for k, (n, frac, base) in enumerate(zip(n_points, outliers, baselines)):
            th = rng.uniform(-0.04, 0.04)
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float32)
            T[:3, 3] = np.array([-base, rng.uniform(-10, 10), rng.uniform(-30, 30)], np.float32)
            X = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n), np.ones(n)], 1) * rng.uniform(300, 12000, (n, 1))
            Xh = np.concatenate([X, np.ones((n, 1))], 1)
            u1 = (K.astype(np.float64) @ Xh[:, :3].T).T
            u2 = (K.astype(np.float64) @ (T[:3].astype(np.float64) @ Xh.T)).T
            p1 = u1[:, :2] / u1[:, 2:] + rng.normal(0, 0.3, (n, 2))
            p2 = u2[:, :2] / u2[:, 2:] + rng.normal(0, 0.3, (n, 2))
            out = rng.random(n) < frac
            p2[out] += rng.uniform(-80, 80, (int(out.sum()), 2))
            wa, wb = rng.permutation(n), rng.permutation(n)
            for f, w, p in ((2 * k, wa, p1), (2 * k + 1, wb, p2)):
                self.kps["x"][f, w], self.kps["y"][f, w] = p[:, 0].astype(np.float32), p[:, 1].astype(np.float32)
                self.counts[f] = n
            self.where.append((wa, wb))
            self.Tcr.append(T)
        self.kf_observed = (rng.random((self.nframes, cap)) < 1 / 3).astype(np.uint8)
        self.view_pos = rng.uniform(-5000, 5000, (self.nframes, cap, 3)).astype(np.float32)

    def row(self, k, n_raw):
        """a match row frame 2k -> frame 2k+1 with n_raw of the correspondences (the same ones for the same arguments)"""
        wa, wb = self.where[k]
        row = np.full(self.cap, -1, np.int32)
        js = np.random.default_rng([k, n_raw]).choice(len(wa), n_raw, replace=False)
        row[wa[js]] = wb[js]
        return row

    def random_row(self, a, b, n_raw, seed):
        """n_raw features of frame a matched to random distinct features of frame b: no geometry behind them"""
        rng = np.random.default_rng([a, b, n_raw, seed])
        row = np.full(self.cap, -1, np.int32)
        row[rng.choice(int(self.counts[a]), n_raw, replace=False)] = rng.choice(int(self.counts[b]), n_raw, replace=False)
        return row

    def pose(self, k):
        """(Trc (12,), P (12,)) of view pair k: rows 0-2 of inv(Tcr), and Kcam * Tcr.rowRange(0,3) in float"""
        T = self.Tcr[k]
        Trc = np.linalg.inv(T.astype(np.float64))[:3].astype(np.float32).reshape(-1)
        return Trc, (K @ T[:3]).astype(np.float32).reshape(-1)


class Batch:
    def __init__(self):
        self.pairs, self.rows, self.Trc, self.P, self.flags = [], [], [], [], []

    def add(self, pair, row, pose, flag=0):
        self.pairs.append(pair); self.rows.append(row); self.Trc.append(pose[0]); self.P.append(pose[1]); self.flags.append(flag)
        return len(self.pairs) - 1

    def take(self, idx):
        b = Batch()
        for p in idx:
            b.add(self.pairs[p], self.rows[p], (self.Trc[p], self.P[p]), self.flags[p])
        return b

    def model(self, tfm, oracle, sc, with_obs=True):
        return tfm.track_batch(oracle, sc.kps, sc.counts, sc.cap, self.pairs, self.rows, self.Trc, self.P, P_REF, LOWER, UPPER,
                               MIN_DEGREE, sc.kf_observed if with_obs else None, sc.view_pos if with_obs else None, self.flags)


# ---- the scene of the direct tests: 12 frames, cap 320 (not a multiple of the 256 threads of a workgroup), counts below cap
CAP, NFRAMES = 320, 12
N_POINTS = (280, 315, 310, 300, 319, 260)
OUTLIERS = (0.3, 0.1, 0.0, 0.0, 0.2, 0.4)
BASELINES = (150.0, 300.0, 80.0, 200.0, 40.0, 120.0)
RAW_COUNTS = (0, 9, 10, 14, 15, 16, 64, 65, 300)
PATHS = (0, 0, 1, 1, 2, 2, 2, 2, 2)
FEW_INLIERS_SEED = 0     # of Scene.random_row(0, 3, 20, .): 20 raw matches whose mask has fewer than 10 inliers, see direct_batch


def main_scene():
    return Scene(CAP, N_POINTS, OUTLIERS, BASELINES)


def direct_batch(sc):
    """-> (batch, names): names[p] says what pair p is there for"""
    b, names = Batch(), {}
    for p, n_raw in enumerate(RAW_COUNTS):
        k = p % 6
        names[b.add((2 * k, 2 * k + 1), sc.row(k, n_raw), sc.pose(k))] = "raw %d" % n_raw
    names[b.add(b.pairs[8], b.rows[8], (b.Trc[8], b.P[8]))] = "repeat of 8"
    same = np.full(CAP, -1, np.int32)
    same[:60] = np.arange(60)
    names[b.add((4, 4), same, sc.pose(2))] = "(f, f)"
    names[b.add((0, 1), sc.row(0, 200), sc.pose(0), flag=1)] = "flagged"
    names[b.add((0, NFRAMES), sc.row(0, 200), sc.pose(0))] = "frame past the end"
    names[b.add((-1, 1), sc.row(0, 200), sc.pose(0))] = "negative frame"
    names[b.add((0, 3), sc.random_row(0, 3, 20, FEW_INLIERS_SEED), sc.pose(0))] = "few inliers"
    names[b.add((0, 1), sc.row(0, 200), sc.pose(0), flag=2)] = "flag without bit 0"
    return b, names


# ---- the scene of the slice test: cap 64, four frames
SLICE_CAP, SLICE_PAIRS = 64, 260


def slice_scene():
    return Scene(SLICE_CAP, (60, 64), (0.1, 0.2), (150.0, 250.0), seed=77)


def slice_batch(sc):
    """260 pairs; every thirteenth and the pairs either side of the slice boundaries have 30..45 raw matches, the others 0..9"""
    b = Batch()
    busy = {0, 99, 100, 129, 130, 131, 244, 245, 246, 259}
    for p in range(SLICE_PAIRS):
        k = p % 2
        n_raw = 30 + p % 16 if (p % 13 == 0 or p in busy) else p % 10
        b.add((2 * k, 2 * k + 1), sc.row(k, n_raw), sc.pose(k))
    return b, sorted(busy)
