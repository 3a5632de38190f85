"""se2gpu_localizer_ba_batch_device on the GPU: the renewal, the gathered arrays, the start pose and the prior against the numpy
model (tests/localizer_ba_model.py); the solve against se2gpu_track_pose_ba and the oracle fed the job's own gathered arrays; every
status and rule once; write-back, independence of the jobs, the statistics' tail, the chain on one stream with one wait, and
the single call's bytes before and after.  nframes = 6, cap = 320, m = 400 (tests/localizer_ba_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import localizer_ba_cases as cases
import localizer_ba_model as model
from test_pose_ba import CX, CY, DELTA, F, TBC, _Twb, _same_run

pytestmark = pytest.mark.gpu

TAIL = 64


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher(0.9)


def _kps(T):
    from se2lam_amd import capi
    k = np.zeros(T["kps_octave"].shape, capi.KP_DTYPE)
    k["x"], k["y"], k["octave"] = T["kps_xy"][..., 0], T["kps_xy"][..., 1], T["kps_octave"]
    return k


class Run:
    """One call on fresh copies of the tables; everything it wrote, read back after one wait.  The work space starts from 0xCD
    bytes (no initialisation is needed), the outputs from sentinels, d_stats lies inside a larger buffer."""

    def __init__(self, matcher, T, jobs, match=None, min_obs=-1, iters=30, optional=True, sync=True):
        from se2lam_amd import capi, localizer as lz
        up = capi.upload
        self.T, self.jobs, self.n, self.matcher = T, list(jobs), len(jobs), matcher
        n = self.n
        (self.nf, self.cap), self.m = T["ftr_mp"].shape, len(T["pos"])
        self.d_Tcw, self.d_Twb = up(T["Tcw"], np.float32), up(T["Twb"], np.float32)
        self.d_kps, self.d_counts = up(_kps(T)), up(T["counts"], np.int32)
        self.d_ftr, self.d_obs = up(T["ftr_mp"], np.int32), up(T["kf_observed"], np.uint8)
        self.d_pos, self.d_null, self.d_good = up(T["pos"], np.float32), up(T["mp_null"], np.uint8), up(T["good_prl"], np.uint8)
        self.d_job = up(np.asarray(jobs, np.int32))
        self.d_match = match if match is None or not isinstance(match, np.ndarray) else up(match, np.int32)
        self.nbytes = lz.ws_bytes(n, self.cap)
        self.d_ws = up(np.full(self.nbytes, 0xCD, np.uint8))
        self.d_status = up(np.full(n, capi.ISENT, np.int32))
        self.d_pose = up(np.full((n, 12), capi.SENT, np.float64))
        self.sb = C.sizeof(capi.BaStats)
        self.d_stats = up(np.full(n * self.sb + TAIL, 0xA5, np.uint8))
        self.d_info = up(np.full((n, 8), capi.ISENT, np.int32))
        self.optional = optional
        o = (lambda d: d) if optional else (lambda d: None)
        lz.do_local_ba_batch_device(matcher, self.d_job, n, self.nf, self.d_Tcw, o(self.d_Twb), self.d_kps, self.d_counts, self.cap,
                                    self.d_ftr, o(self.d_obs), self.d_match, self.d_pos, self.m, o(self.d_null), o(self.d_good),
                                    T["inv_level_sigma2"], T["K"], T["Tbc12"], T["huber"], self.d_ws, self.d_status, self.d_pose,
                                    o(self.d_stats), self.d_info, xrot_info=T["xrot_info"], yrot_info=T["yrot_info"], z_info=T["z_info"],
                                    iters=iters, min_obs=min_obs)
        if sync:
            matcher.sync()
            self.read()

    def read(self):
        from se2lam_amd import capi, localizer as lz
        from se2lam_amd.optimizer import _stats_dict
        n = self.n
        self.status = self.d_status.to_numpy(np.int32, (n,))
        self.pose = self.d_pose.to_numpy(np.float64, (n, 12))
        self.info = self.d_info.to_numpy(np.int32, (n, 8))
        self.raw = self.d_ws.to_numpy(np.uint8, (self.nbytes,))
        self.lay = lz.ws_layout(n, self.cap)
        self.stats_raw = self.d_stats.to_numpy(np.uint8, (n * self.sb + TAIL,))
        self.stats = [_stats_dict(capi.BaStats.from_buffer_copy(self.stats_raw[i * self.sb:(i + 1) * self.sb].tobytes())) for i in range(n)]
        self.Tcw = self.d_Tcw.to_numpy(np.float32, (self.nf, 12))
        self.Twb = self.d_Twb.to_numpy(np.float32, (self.nf, 3))
        self.ftr_mp = self.d_ftr.to_numpy(np.int32, (self.nf, self.cap))
        self.kf_observed = self.d_obs.to_numpy(np.uint8, (self.nf, self.cap))
        return self

    def gather(self, b):
        from se2lam_amd import localizer as lz
        return lz.read_gather(self.raw, self.lay, b)

    def slices(self, b):
        """the bytes of job b's slice of every gathered array, whole strides"""
        return [self.raw[o + s * b:o + s * (b + 1)].copy() for o, s in (self.lay[k] for k in self.lay)]


@pytest.fixture(scope="module")
def plain(matcher):
    """all six frames without a match row, the gate off: 0, 6, 37, 257, 300 and 31 edges"""
    return Run(matcher, cases.tables(), range(cases.NFRAMES))


@pytest.fixture(scope="module")
def renewed(matcher):
    """frames 1-5 with match rows that exercise every renewal rule; frame 0 is no job's"""
    T = cases.tables()
    frames = [5, 1, 4, 2, 3]
    r = Run(matcher, T, frames, cases.match_rows(T, frames))
    r.rows = cases.match_rows(T, frames)
    return r


def _check_gather(r, b, want):
    g = r.gather(b)
    assert np.array_equal(g["counts"], want["info"]) and np.array_equal(r.info[b], want["info"]), (b, g["counts"], want["info"])
    for k in ("e_ftr", "xyz", "uv", "w"):
        assert np.array_equal(g[k], want[k]), (b, k)
    assert np.array_equal(g["pose0"][9:], want["pose0"][9:])
    assert np.allclose(g["pose0"][:9], want["pose0"][:9], rtol=0, atol=1e-12)
    assert np.allclose(g["prior_meas"], want["prior_meas"], rtol=0, atol=1e-12)
    assert np.allclose(g["prior_info"], want["prior_info"], rtol=1e-13, atol=0)
    return g


def test_gathered_arrays_and_renewal_against_the_model(plain, renewed):
    assert plain.status.tolist() == [0] * 6 and renewed.status.tolist() == [0] * 5
    assert plain.info[:, 2].tolist() == list(cases.EDGES)
    for b, f in enumerate(plain.jobs):
        _check_gather(plain, b, model.job(plain.T, f, None, -1))
    assert np.array_equal(plain.ftr_mp, plain.T["ftr_mp"]) and np.array_equal(plain.kf_observed, plain.T["kf_observed"])
    ftr, obs = renewed.T["ftr_mp"].copy(), renewed.T["kf_observed"].copy()
    for b, f in enumerate(renewed.jobs):
        want = model.job(renewed.T, f, renewed.rows[b], -1)
        _check_gather(renewed, b, want)
        assert want["info"][3] >= 3 and want["info"][4] >= 1
        ftr[f], obs[f] = want["ftr_mp"], want["kf_observed"]
    assert np.array_equal(renewed.ftr_mp, ftr) and np.array_equal(renewed.kf_observed, obs)       # frame 0's rows included


def _solve_both(oracle, g):
    from se2lam_amd.localizer import Localizer
    loc = Localizer()
    args = (cases.matrix(g["pose0"]), cases.matrix(g["prior_meas"]), g["prior_info"], g["xyz"], g["uv"], g["w"], F, CX, CY, DELTA, 30)
    T1 = loc.pose_ba(*args)
    To, so = oracle.pose_only_ba(*args)
    return T1, loc.stats, To, so


def _same_pose(p12, T):
    P = cases.matrix(p12)
    assert np.allclose(P[:3, :3], T[:3, :3], atol=1e-7) and np.allclose(P[:3, 3], T[:3, 3], rtol=1e-5, atol=1e-3)


def test_solve_against_the_single_call_and_the_oracle(matcher, oracle, plain, renewed):
    """fed the job's own gathered arrays read back from the work space"""
    reject = Run(matcher, cases.tables(shift_uv=cases.REJECT), [cases.REJECT[0]])
    assert reject.status.tolist() == [0] and max(reject.stats[0]["trials_hist"]) > 1        # LM rejected trials
    equal_bits = []
    for r in (plain, renewed, reject):
        for b, f in enumerate(r.jobs):
            g = r.gather(b)
            T1, s1, To, so = _solve_both(oracle, g)
            if len(g["e_ftr"]) == 0:            # only the prior, which the start pose satisfies: the cost is round-off, the pose compares
                assert np.allclose(cases.matrix(r.pose[b]), To, atol=1e-9) and np.allclose(cases.matrix(r.pose[b]), T1, atol=1e-9)
                continue
            assert f in cases.HISTORY_FRAMES
            print("job", b, "frame", f, "edges", len(g["e_ftr"]), "iterations", r.stats[b]["iterations"], "chi2", r.stats[b]["chi2_init"], "->",
                  r.stats[b]["chi2_final"], "trials", r.stats[b]["trials_hist"])
            _same_run(r.stats[b], s1)
            _same_run(r.stats[b], so)
            _same_pose(r.pose[b], T1)
            _same_pose(r.pose[b], To)
            equal_bits.append(bool(np.array_equal(cases.matrix(r.pose[b]), T1)))
    print("poses equal to se2gpu_track_pose_ba's to the bit:", equal_bits)                   # recorded, not a pass condition


def test_every_status_and_rule_once(matcher):
    T = cases.tables(edges=(26, 27, 30, 31, 6, 6))          # + 2 null + 2 bad parallax: 30, 31, 34, 35 observations
    r = Run(matcher, T, [cases.NFRAMES, 0, 1, -1], min_obs=30)
    assert r.status.tolist() == [1, 5, 0, 1]
    from se2lam_amd import capi
    assert (r.info[0] == 0).all() and (r.info[3] == 0).all() and (r.pose[[0, 3]] == capi.SENT).all()
    assert r.info[1, 1] == 30 and r.info[2, 1] == 31 and r.info[1, 2] == 26
    # status 5: the start pose comes back, the table rows stay, the statistics are zero, the gathered arrays are there
    want = model.job(T, 0, None, 30)
    assert want["status"] == 5
    _check_gather(r, 1, want)
    assert np.array_equal(r.pose[1][9:], want["pose0"][9:]) and np.allclose(r.pose[1], want["pose0"], rtol=0, atol=1e-12)
    assert np.array_equal(r.pose[1], r.gather(1)["pose0"])
    assert np.array_equal(r.Tcw[[0, 2, 3, 4, 5]], T["Tcw"][[0, 2, 3, 4, 5]]) and np.array_equal(r.Twb[[0, 2, 3, 4, 5]], T["Twb"][[0, 2, 3, 4, 5]])
    assert not r.stats_raw[:r.sb].any() and not r.stats_raw[r.sb:2 * r.sb].any() and not r.stats_raw[3 * r.sb:4 * r.sb].any()
    assert r.stats[2]["iterations"] >= 2 and not np.array_equal(r.Tcw[1], T["Tcw"][1])
    # the gate off: the same frame runs
    assert Run(matcher, T, [0], min_obs=-1).status.tolist() == [0] and Run(matcher, T, [0], min_obs=29).status.tolist() == [0]

    # a duplicate, a null and a bad-parallax point, entries outside the table, octaves outside the levels
    T = cases.tables()
    f = 3
    n = int(T["counts"][f])
    free = np.nonzero(T["ftr_mp"][f, :n] < 0)[0]
    held = np.nonzero((T["ftr_mp"][f, :n] >= 0) & (T["ftr_mp"][f, :n] < cases.GOOD))[0]
    T["ftr_mp"][f, free[0]], T["ftr_mp"][f, free[1]] = cases.M + 7, -5
    T["ftr_mp"][f, free[2]] = T["ftr_mp"][f, held[0]]
    T["ftr_mp"][f, free[3]] = T["ftr_mp"][f, held[-1]]
    T["kps_octave"][f, held[5]], T["kps_octave"][f, held[9]] = cases.NLEVELS, -1
    want = model.job(T, f, None, -1)
    assert want["info"].tolist() == [n, 257 + 4, 255, 0, 2, 3, 0, 0]
    r = Run(matcher, T, [f])
    assert r.status.tolist() == [0]
    g = _check_gather(r, 0, want)
    assert free[2] in g["e_ftr"] or held[0] in g["e_ftr"]

    # iters = 0: the pose comes back, the table row is the float of the start pose
    T = cases.tables()
    r = Run(matcher, T, [2], iters=0)
    assert r.status.tolist() == [0] and r.stats[0]["iterations"] == 0
    assert np.array_equal(r.pose[0], r.gather(0)["pose0"]) and np.array_equal(r.Tcw[2], model.tcw_row_of(r.pose[0]))

    # every optional table left out: no point is null, all are good, nothing but the pose is written
    T2 = dict(T, mp_null=np.zeros(cases.M, np.uint8), good_prl=np.ones(cases.M, np.uint8))
    r = Run(matcher, T, [4], optional=False)
    assert r.status.tolist() == [0]
    _check_gather(r, 0, model.job(T2, 4, None, -1))
    assert r.info[0, 2] == 304 and (r.stats_raw == 0xA5).all() and np.array_equal(r.Twb, T["Twb"]) and np.array_equal(r.kf_observed, T["kf_observed"])


def test_a_row_longer_than_one_staged_chunk(matcher):
    """cap = 4,300 > the 4,096 features the kernel stages in LDS at a time: duplicates inside the first chunk, inside the second and
    across the two, edges on both sides of the boundary; the gather alone (iters = 0)"""
    base = cases.tables()
    nf, cap, m, f, n = 2, 4300, 50, 1, 4250
    rng = np.random.default_rng(3)
    T = dict(base, Tcw=base["Tcw"][:nf].copy(), Twb=base["Twb"][:nf].copy(), kps_xy=rng.uniform(0, 640, (nf, cap, 2)).astype(np.float32),
             kps_octave=rng.integers(0, cases.NLEVELS, (nf, cap)).astype(np.int32), counts=np.array([0, n], np.int32),
             ftr_mp=np.full((nf, cap), -1, np.int32), kf_observed=np.zeros((nf, cap), np.uint8), pos=base["pos"][:m].copy(),
             mp_null=np.zeros(m, np.uint8), good_prl=np.ones(m, np.uint8))
    T["mp_null"][48], T["good_prl"][49] = 1, 0
    ftrs = np.concatenate([[0, 5, 10, 4000, 4095, 4096, 4097, 4100, 4200, 4249], rng.choice(np.arange(20, 3990), 15, replace=False),
                           rng.choice(np.arange(4101, 4199), 15, replace=False)])
    T["ftr_mp"][f, ftrs] = np.arange(len(ftrs))                   # points 0..39
    T["ftr_mp"][f, 4000] = T["ftr_mp"][f, 5]                       # inside the first chunk
    T["ftr_mp"][f, 4249] = T["ftr_mp"][f, 4100]                    # inside the second
    T["ftr_mp"][f, 4200] = T["ftr_mp"][f, 10]                      # across
    T["ftr_mp"][f, 4096] = T["ftr_mp"][f, 4095]                    # across, neighbours
    T["ftr_mp"][f, [7, 4150]] = 48, 49                            # a null and a bad-parallax point
    T["ftr_mp"][f, n:] = 3                                         # past counts: never read
    want = model.job(T, f, None, -1)
    assert want["info"].tolist() == [n, 38, 36, 0, 4, 0, 0, 0]
    r = Run(matcher, T, [f, 0], iters=0)
    assert r.status.tolist() == [0, 0] and r.info[1].tolist() == [0] * 8
    g = _check_gather(r, 0, want)
    assert {4000, 4249, 4200, 4096} <= set(g["e_ftr"].tolist()) and not {5, 4100, 10, 4095} & set(g["e_ftr"].tolist())


def test_write_back(plain, renewed):
    for r in (plain, renewed):
        for b, f in enumerate(r.jobs):
            assert np.array_equal(r.Tcw[f], model.tcw_row_of(r.pose[b])) and np.array_equal(r.Tcw[f], r.pose[b][[0, 1, 2, 9, 3, 4, 5, 10, 6, 7, 8, 11]].astype(np.float32))
            want = model.twb_of(r.pose[b], r.T["Tbc12"])
            assert (np.abs(r.Twb[f].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), (f, r.Twb[f], want)
            # and the pose it describes is the frame's true one to the accuracy of test_oracle_pose_only_ba_recovers_the_pose
            if len(r.gather(b)["e_ftr"]) >= 257:
                assert np.abs(r.Twb[f][:2] - r.T["true_pose"][f][:2]).max() < 8.0
    assert np.array_equal(renewed.Tcw[0], renewed.T["Tcw"][0]) and np.array_equal(renewed.Twb[0], renewed.T["Twb"][0])


def test_a_job_depends_on_that_job_alone(matcher):
    T = cases.tables()
    rows = cases.match_rows(T, [3, 1, 2])
    runs = [(Run(matcher, T, [3], rows[[0]]), 0), (Run(matcher, T, [3, 1, 2], rows), 0), (Run(matcher, T, [1, 2, 3], rows[[1, 2, 0]]), 2),
            (Run(matcher, T, [3], rows[[0]]), 0)]
    a, ia = runs[0]
    assert a.status[ia] == 0 and a.info[ia, 3] >= 3
    for r, i in runs[1:]:
        for x, y in zip(a.slices(ia), r.slices(i)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.pose[ia], r.pose[i]) and np.array_equal(a.info[ia], r.info[i]) and a.status[ia] == r.status[i]
        assert np.array_equal(a.stats_raw[ia * a.sb:(ia + 1) * a.sb], r.stats_raw[i * r.sb:(i + 1) * r.sb])
        assert np.array_equal(a.Tcw[3], r.Tcw[3]) and np.array_equal(a.Twb[3], r.Twb[3])
        assert np.array_equal(a.ftr_mp[3], r.ftr_mp[3]) and np.array_equal(a.kf_observed[3], r.kf_observed[3])


def test_the_bytes_behind_the_statistics_stay(plain, renewed):
    for r in (plain, renewed):
        assert (r.stats_raw[r.n * r.sb:] == 0xA5).all() and len(r.stats_raw) == r.n * r.sb + TAIL
        assert r.stats[r.n - 1]["iterations"] >= 1


def _scene_for(T, f, seed=5):
    """descriptors for frame f's features and the map's points, so that MatchByProjection at the frame's start pose finds the points
    again whose observations were taken away"""
    rng = np.random.default_rng(seed)
    n = int(T["counts"][f])
    T = dict(T, ftr_mp=T["ftr_mp"].copy(), kf_observed=T["kf_observed"].copy())
    mp_desc = rng.integers(0, 256, (cases.M, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (cases.CAP, 32), dtype=np.uint8)
    mp_octave = rng.integers(0, cases.NLEVELS, cases.M).astype(np.int32)
    held = np.nonzero((T["ftr_mp"][f, :n] >= 0) & (T["ftr_mp"][f, :n] < cases.GOOD))[0]
    pts = T["ftr_mp"][f, held]
    desc[held] = mp_desc[pts] ^ np.packbits(rng.random((len(held), 256)) < 0.02, axis=1)
    mp_octave[pts] = T["kps_octave"][f, held]
    lost = held[::4]                                               # a quarter of the observations is taken away
    T["ftr_mp"][f, lost] = -1
    T["kf_observed"][f, lost] = 0
    return T, mp_desc, desc, mp_octave


def test_the_chain_with_one_wait(matcher):
    """se2gpu_match_projection_device -> this call on its row -> se2gpu_covis_build_device / _pairs_device, one stream, one wait"""
    from se2lam_amd import capi, covis, localizer as lz
    up = capi.upload
    f = 4
    T, mp_desc, desc, mp_octave = _scene_for(cases.tables(), f)
    Tcw_seen = np.linalg.inv(_Twb(*T["true_pose"][f]) @ TBC)[:3, :4].astype(np.float32)    # the matcher's pose argument is the host's
    live = np.where(np.arange(cases.CAP)[None] < T["counts"][:, None], T["ftr_mp"], -1)      # the key frames' side as a CSR
    lists = [tuple(x.astype(np.int32) for x in np.nonzero(live == p)) for p in range(cases.M)]
    mp_ptr, obs_frame, obs_ftr = capi.csr(lists)
    results = []
    for wait in (False, True):
        sync = matcher.sync if wait else (lambda: None)
        kps = _kps(T)
        d = dict(Tcw=up(T["Tcw"], np.float32), Twb=up(T["Twb"], np.float32), kps=up(kps), counts=up(T["counts"], np.int32),
                 ftr=up(T["ftr_mp"], np.int32), obs=up(T["kf_observed"], np.uint8), pos=up(T["pos"], np.float32), null=up(T["mp_null"], np.uint8),
                 good=up(T["good_prl"], np.uint8), job=up(np.array([f], np.int32)), mp_desc=up(mp_desc), mp_oct=up(mp_octave, np.int32),
                 desc=up(desc), idx=up(np.full(cases.CAP, -7, np.int32)), nm=up(np.full(1, -7, np.int32)),
                 ws=up(np.full(lz.ws_bytes(1, cases.CAP), 0xCD, np.uint8)), status=up(np.full(1, capi.ISENT, np.int32)),
                 pose=up(np.full(12, capi.SENT, np.float64)), info=up(np.full(8, capi.ISENT, np.int32)))
        cv = covis.DeviceCovis(T["counts"], cases.CAP, mp_ptr, obs_frame, obs_ftr, T["mp_null"], T["good_prl"])
        row = f * cases.CAP
        matcher.match_projection_device(d["pos"].ptr, d["mp_desc"].ptr, d["mp_oct"].ptr, d["null"].ptr, cases.M, Tcw_seen, (F, F, CX, CY),
                                        d["kps"].ptr.value + row * kps.dtype.itemsize, d["desc"].ptr, d["obs"].ptr.value + row, cases.CAP,
                                        15, 2, d["idx"].ptr, d["nm"].ptr)
        sync()
        lz.do_local_ba_batch_device(matcher, d["job"], 1, cases.NFRAMES, d["Tcw"], d["Twb"], d["kps"], d["counts"], cases.CAP, d["ftr"], d["obs"],
                                    d["idx"], d["pos"], cases.M, d["null"], d["good"], T["inv_level_sigma2"], T["K"], T["Tbc12"], T["huber"],
                                    d["ws"], d["status"], d["pose"], None, d["info"], min_obs=30)
        sync()
        cv.build(matcher, sync=wait)
        pairs = covis.pairs_device(matcher, cv, [f, f], [3, 5], sync=wait)
        matcher.sync()                                              # the one wait of the chain
        pr = pairs if wait else pairs.read()
        results.append(dict(idx=d["idx"].to_numpy(np.int32, (cases.CAP,)), nm=d["nm"].to_numpy(np.int32, (1,)),
                            status=d["status"].to_numpy(np.int32, (1,)), pose=d["pose"].to_numpy(np.float64, (12,)),
                            info=d["info"].to_numpy(np.int32, (8,)), Tcw=d["Tcw"].to_numpy(np.float32, (cases.NFRAMES, 12)),
                            Twb=d["Twb"].to_numpy(np.float32, (cases.NFRAMES, 3)), ftr=d["ftr"].to_numpy(np.int32, (cases.NFRAMES, cases.CAP)),
                            obs=d["obs"].to_numpy(np.uint8, (cases.NFRAMES, cases.CAP)), bits=cv.read_bits(), size=cv.read_size_obs(),
                            pair_out=pr["out"], ratio=pr["ratio"]))
    a, b = results
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["status"].tolist() == [0] and a["nm"][0] > 20 and a["info"][3] == a["nm"][0]          # every match renewed an observation
    want = model.job(T, f, a["idx"], 30)
    assert np.array_equal(a["info"], want["info"]) and np.array_equal(a["ftr"][f], want["ftr_mp"]) and np.array_equal(a["obs"][f], want["kf_observed"])


def test_the_single_call_is_untouched(matcher, plain):
    from se2lam_amd.localizer import Localizer
    g = plain.gather(3)
    args = (cases.matrix(g["pose0"]), cases.matrix(g["prior_meas"]), g["prior_info"], g["xyz"], g["uv"], g["w"], F, CX, CY, DELTA, 30)
    loc = Localizer()
    T0, s0 = loc.pose_ba(*args), loc.stats
    assert loc.stats_tail_intact
    Run(matcher, cases.tables(), [3, 4])
    T1, s1 = loc.pose_ba(*args), loc.stats
    assert T0.tobytes() == T1.tobytes() and s0 == s1 and loc.stats_tail_intact


# ---- a camera off the body's axes ----------------------------------------------------------------------------------------------

def test_off_axis_camera_gather_prior_solve_and_write_back(matcher, oracle):
    """the tables of `plain` (the same random draws) seen through synth.OFF_AXIS_TBC / OFF_CENTRE_CAM: adj(Tbc) in the plane-motion
    prior's information and Tbc in its measurement are full matrices, the principal point is off the image centre.  The checks of
    test_gathered_arrays_and_renewal_against_the_model, test_solve_against_the_single_call_and_the_oracle and test_write_back."""
    from se2lam_amd import synth
    from se2lam_amd.localizer import Localizer
    f_, cx, cy = synth.OFF_CENTRE_CAM
    T = cases.tables(Tbc=synth.OFF_AXIS_TBC, cam=synth.OFF_CENTRE_CAM)
    assert np.abs(T["Tbc12"][:9]).min() > 0.02 and T["K"][0, 0] == np.float32(f_) and T["K"][1, 2] == np.float32(cy)
    r = Run(matcher, T, range(cases.NFRAMES))
    assert r.status.tolist() == [0] * 6 and r.info[:, 2].tolist() == list(cases.EDGES)
    for b, f in enumerate(r.jobs):
        g = _check_gather(r, b, model.job(T, f, None, -1))
        # the prior against the definitions (tests/independent.py), at test_track_independent.py's bounds
        import independent as ind
        mn, infn = ind.plane_motion_prior_numpy(cases.matrix(g["pose0"]), synth.OFF_AXIS_TBC)
        assert np.allclose(g["prior_info"].reshape(6, 6), infn, rtol=1e-12, atol=0)
        assert np.allclose(cases.matrix(g["prior_meas"]), mn, atol=1e-9)
        loc = Localizer()
        args = (cases.matrix(g["pose0"]), cases.matrix(g["prior_meas"]), g["prior_info"], g["xyz"], g["uv"], g["w"], float(T["K"][0, 0]),
                float(T["K"][0, 2]), float(T["K"][1, 2]), DELTA, 30)
        T1 = loc.pose_ba(*args)
        To, so = oracle.pose_only_ba(*args)
        if len(g["e_ftr"]) == 0:
            assert np.allclose(cases.matrix(r.pose[b]), To, atol=1e-9) and np.allclose(cases.matrix(r.pose[b]), T1, atol=1e-9)
        else:
            _same_run(r.stats[b], loc.stats)
            _same_run(r.stats[b], so)
            _same_pose(r.pose[b], T1)
            _same_pose(r.pose[b], To)
        assert np.array_equal(r.Tcw[f], model.tcw_row_of(r.pose[b]))
        want = model.twb_of(r.pose[b], T["Tbc12"])
        assert (np.abs(r.Twb[f].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), (f, r.Twb[f], want)
        if len(g["e_ftr"]) >= 257:
            assert np.abs(r.Twb[f][:2] - T["true_pose"][f][:2]).max() < 8.0
