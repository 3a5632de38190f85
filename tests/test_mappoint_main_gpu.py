"""se2gpu_mappoint_main_batch_device and se2gpu_match_projection_device on the GPU: every output against the numpy model
(tests/mappoint_main_model.py), EXACTLY - the distances are IEEE operations on both sides.  One frame set and one model
run are shared; every device run is one small batch."""
import numpy as np
import pytest

import mappoint_main_cases as mc
import mappoint_main_model as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fs():
    return mc.FrameSet()


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


def _device_frames(fs, kps=None, null=None):
    from se2lam_amd import mappoint as mpt
    return mpt.DeviceFrames(fs.kps if kps is None else kps, fs.desc, fs.counts, mc.CAP, fs.null if null is None else null, fs.view)


@pytest.fixture(scope="module")
def dframes(fs):
    return _device_frames(fs)


def _device(matcher, dframes, lists, prev=None, view=True):
    from se2lam_amd import mappoint as mpt
    b = mpt.MainBatch(lists, prev, mc.sentinels(max(len(lists), 1)))
    b.run(matcher, dframes, mc.SCALE, view)
    return b.download(matcher)


def _model(fs, lists, prev=None, view=True, kps=None, null=None):
    ptr, fr, ft = mc.csr(lists)
    a = fs.model_args(null=null, view=view)
    if kps is not None:
        a["kps"] = kps
    return mm.update_main_batch(mp_ptr=ptr, obs_frame=fr, obs_ftr=ft, prev_main_frame=prev, out=mc.sentinels(len(lists)), **a)


def _same(got, want, what=""):
    for k in ("info", "main_desc", "main_frame", "main_octave"):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1)))
    assert np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32)), (what, "dist")


@pytest.fixture(scope="module")
def first(fs, matcher, dframes):
    lists = mc.first_batch(fs)
    return lists, _model(fs, lists), _device(matcher, dframes, lists)


def test_first_batch_equals_the_model(first):
    lists, want, got = first
    lens = [len(f) for f, _ in lists]
    assert set(mc.BATCH_N) <= set(lens) and 0 in lens and len(lists) == 40
    assert want["info"][lens.index(0)].tolist() == [-1, 0, 0, 0] and want["main_frame"][lens.index(0)] == -55
    assert (want["info"][:, 2] == lens).all() and (want["info"][:, 3] == (np.array(lens) > 0)).all()
    _same(got, want)


def test_beyond_the_register_tiles(fs, matcher, dframes):
    """more than 256 observations: the tiles past the ones a wave keeps in registers are recomputed from memory"""
    rng = np.random.default_rng(5)
    lists = [fs.pick(rng, n) for n in (257, 300, 256, 450)]
    _same(_device(matcher, dframes, lists), _model(fs, lists))


def test_ties(fs, matcher, dframes):
    """observations that are copies of 2 or 3 distinct descriptors, or of one: several rows share the least median, the first
    in list order wins; the reversed list picks the mirrored place where the winner's descriptor is unique in the list"""
    rng = np.random.default_rng(9)
    base = fs.pick(rng, 3)
    lists = []
    for n, ndist in ((6, 2), (7, 3), (8, 2), (9, 3), (20, 2), (40, 3), (70, 2), (135, 3), (5, 1), (33, 1), (100, 1)):
        sel = rng.integers(0, ndist, n)
        sel[:ndist] = np.arange(ndist)
        lists.append((base[0][sel], base[1][sel]))
    mirrored = [fs.pick(rng, n) for n in (2, 3, 8, 16, 33, 64, 130)]
    lists += mirrored + [(f[::-1].copy(), k[::-1].copy()) for f, k in mirrored]
    want = _model(fs, lists)
    assert (want["info"][8:11, :2] == 0).all()             # all-identical descriptors: place 0, median 0
    got = _device(matcher, dframes, lists)
    _same(got, want)
    nm = len(mirrored)
    for i, (f, k) in enumerate(mirrored):
        a, b = got["info"][11 + i], got["info"][11 + nm + i]
        D = mm.distance_table(fs.desc[f * mc.CAP + k])
        med = np.sort(D, 1)[:, (len(f) - 1) // 2]
        if (med == med.min()).sum() == 1:                  # a unique least median: the same observation from the other end
            assert b[0] == len(f) - 1 - a[0] and b[1] == a[1]
        else:                                              # a tie: each direction takes its own first
            assert a[0] == np.flatnonzero(med == med.min())[0] and b[0] == len(f) - 1 - np.flatnonzero(med == med.min())[-1]
    assert got["info"][11][0] == 0 and got["info"][11 + nm][0] == 0   # N = 2 always ties: place 0 from both ends


def test_skipping(fs, matcher):
    """null frames, frame indices -1 and nframes, feature indices at counts and at cap: the result is the model's on the
    valid observations alone, places counted in the full list; what the call leaves alone keeps its sentinel"""
    rng = np.random.default_rng(13)
    null = np.zeros(mc.NFRAMES, np.uint8)
    null[[20, 21, 22, 23, 24]] = 1
    def pick(n):                                            # n observations in frames that are not null
        f, k = fs.pick(rng, n + 40)
        keep = ~np.isin(f, np.flatnonzero(null))
        return f[keep][:n].copy(), k[keep][:n].copy()
    f, k = pick(9)
    f[4] = 20                                               # a null frame in the middle
    bad_f = np.array([-1, mc.NFRAMES, 2, 0, 1], np.int32)   # frame 2 has 10 features, frame 1 counts 19 > cap
    bad_k = np.array([0, 0, 10, mc.CAP, mc.CAP], np.int32)
    g, h = pick(70)
    lists = [(f, k),
             (np.array([20, 21, 22, 23], np.int32), np.zeros(4, np.int32)),            # every frame null
             (np.concatenate([bad_f, f[:3]]), np.concatenate([bad_k, k[:3]])),
             (bad_f, bad_k),                                                            # nothing valid at all
             (np.insert(g, [0, 30, 66], [-1, 22, mc.NFRAMES]).astype(np.int32), np.insert(h, [0, 30, 66], [0, 0, 0]).astype(np.int32))]
    want = _model(fs, lists, null=null)
    assert want["info"][:, 2].tolist() == [8, 0, 3, 0, 70] and want["info"][2, 0] >= 5
    got = _device(matcher, _device_frames(fs, null=null), lists)
    _same(got, want)
    for p in (1, 3):
        assert got["info"][p].tolist() == [-1, 0, 0, 0] and got["main_frame"][p] == -55 and (got["main_desc"][p] == 0xAB).all()
        assert got["main_octave"][p] == -77 and (got["dist"][p] == -1.0).all()
    ptr, fr, ft = mc.csr(lists)
    valid = [(fr[ptr[p]:ptr[p + 1]][mm.valid_observations(fr[ptr[p]:ptr[p + 1]], ft[ptr[p]:ptr[p + 1]], fs.counts, mc.CAP, mc.NFRAMES, null)],
              ft[ptr[p]:ptr[p + 1]][mm.valid_observations(fr[ptr[p]:ptr[p + 1]], ft[ptr[p]:ptr[p + 1]], fs.counts, mc.CAP, mc.NFRAMES, null)])
             for p in (0, 2, 4)]
    only = _model(fs, valid, null=null)
    for i, p in enumerate((0, 2, 4)):
        assert np.array_equal(only["main_desc"][i], got["main_desc"][p]) and only["main_frame"][i] == got["main_frame"][p]
        assert only["info"][i, 1:].tolist() == got["info"][p, 1:].tolist()


def test_changed(fs, matcher, dframes, first):
    lists, want0, _ = first
    m = len(lists)
    has = want0["info"][:, 0] >= 0
    same = want0["main_frame"].copy()
    got = _device(matcher, dframes, lists, prev=same)       # mMainKF stays: :280 returns early
    _same(got, _model(fs, lists, prev=same))
    assert (got["info"][has, 3] == 0).all() and (got["main_octave"] == -77).all() and (got["dist"] == -1.0).all()
    assert np.array_equal(got["main_desc"], want0["main_desc"])
    other = np.where(same == 5, 6, 5).astype(np.int32)
    got = _device(matcher, dframes, lists, prev=other)
    _same(got, _model(fs, lists, prev=other))
    assert (got["info"][has, 3] == 1).all() and (got["main_octave"][has] >= 0).all() and (got["dist"][has] != -1.0).all()
    # an octave of nlevels: bit 1, the octave is written, the distances are not
    kps = fs.kps.copy()
    q = int(np.flatnonzero(has)[3])
    ptr, fr, ft = mc.csr(lists)
    off = int(want0["main_frame"][q]) * mc.CAP + int(ft[ptr[q] + want0["info"][q, 0]])
    kps["octave"][off] = mc.NLEVELS
    got = _device(matcher, _device_frames(fs, kps=kps), lists)
    _same(got, _model(fs, lists, kps=kps))
    assert got["info"][q, 3] == 3 and got["main_octave"][q] == mc.NLEVELS and (got["dist"][q] == -1.0).all()
    # no view positions: no distances
    got = _device(matcher, dframes, lists, view=False)
    _same(got, _model(fs, lists, view=False))
    assert (got["dist"] == -1.0).all() and (got["main_octave"][has] >= 0).all()


def test_independence(fs, matcher, dframes, first):
    lists, _, got0 = first
    perm = np.random.default_rng(2).permutation(len(lists))
    got = _device(matcher, dframes, [lists[i] for i in perm])
    _same(got, {k: v[perm] for k, v in got0.items()}, "shuffled")
    lens = [len(f) for f, _ in lists]
    for n in (2, 33, 130):
        p = lens.index(n)
        alone = _device(matcher, dframes, [lists[p]])
        _same(alone, {k: v[p:p + 1] for k, v in got0.items()}, "alone %d" % n)
    again = _device(matcher, dframes, lists)
    for k in got0:
        assert got0[k].tobytes() == again[k].tobytes(), k


def test_empty_batch_and_empty_observation_arrays(fs, matcher, dframes):
    assert _device(matcher, dframes, [])["info"].shape == (0, 4)
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    got = _device(matcher, dframes, [e, e, e])
    assert (got["info"] == [-1, 0, 0, 0]).all() and (got["main_frame"] == -55).all()


def _scene(seed=4, n=900, m=700):
    """one key frame of n features on a jittered grid and m map points that project onto some of them (after
    tests/test_match_gpu.py's MatchByProjection case, without the extractor)"""
    from se2lam_amd import capi
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, capi.KP_DTYPE)
    kps["x"] = rng.uniform(20, 620, n).astype(np.float32)
    kps["y"] = rng.uniform(20, 460, n).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n)
    kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fx = fy = 400.0; cx, cy = 320.0, 240.0
    src = rng.integers(0, n, m)
    depth = rng.uniform(800, 6000, m).astype(np.float32)
    Xc = np.stack([(kps["x"][src] + rng.normal(0, 2, m) - cx) / fx * depth, (kps["y"][src] + rng.normal(0, 2, m) - cy) / fy * depth,
                   depth], 1).astype(np.float32)
    th = 0.01
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float32)
    t = np.array([15.0, -4.0, 8.0], np.float32)
    Tcw = np.concatenate([R, t[:, None]], 1).astype(np.float32)
    mp_pos = ((Xc - t) @ R).astype(np.float32)
    mp_desc = desc[src] ^ np.packbits(rng.random((m, 256)) < 0.03, axis=1)
    mp_octave = np.clip(kps["octave"][src] + rng.integers(-1, 2, m), 0, 7).astype(np.int32)
    mp_skip = (rng.random(m) < 0.1).astype(np.uint8)
    kf_obs = (rng.random(n) < 0.2).astype(np.uint8)
    return mp_pos, mp_desc, mp_octave, mp_skip, Tcw, (fx, fy, cx, cy), kps, desc, kf_obs


def _projection_device(matcher, d_pos, d_desc, d_oct, d_skip, m, Tcw, K4, kps, desc, kf_obs):
    from se2lam_amd import capi
    up = capi.DeviceArray.from_numpy
    n = len(kps)
    d_kps, d_kd, d_obs = up(kps), up(desc), up(kf_obs)
    d_idx, d_nm = up(np.full(n, -7, np.int32)), up(np.full(1, -7, np.int32))
    matcher.match_projection_device(d_pos.ptr, d_desc.ptr, d_oct.ptr, d_skip.ptr, m, Tcw, K4, d_kps.ptr, d_kd.ptr, d_obs.ptr, n,
                                    15, 2, d_idx.ptr, d_nm.ptr)
    matcher.sync()
    return int(d_nm.to_numpy(np.int32, (1,))[0]), d_idx.to_numpy(np.int32, (n,))


def test_chain_projection_on_device_arrays(matcher):
    from se2lam_amd import capi, mappoint as mpt
    up = capi.DeviceArray.from_numpy
    mp_pos, mp_desc, mp_octave, mp_skip, Tcw, K4, kps, desc, kf_obs = _scene()
    m = len(mp_octave)
    nm_h, idx_h = matcher.MatchByProjection(mp_pos, mp_desc, mp_octave, mp_skip, Tcw, K4, kps, desc, kf_obs, 15, 2)
    assert nm_h > 100
    nm_d, idx_d = _projection_device(matcher, up(mp_pos), up(mp_desc), up(mp_octave), up(mp_skip), m, Tcw, K4, kps, desc, kf_obs)
    assert nm_d == nm_h and np.array_equal(idx_d, idx_h)

    # the same with mp_desc / mp_octave taken straight from the batch call's outputs: map point p is observed by 1..6 frames
    # of a small frame set whose features carry noisy copies of its descriptor
    rng = np.random.default_rng(8)
    nobs_p = rng.integers(1, 7, m)
    cap = 64
    nfr = int(np.ceil(nobs_p.sum() / cap)) + 1
    slot = rng.permutation(nfr * cap)[:nobs_p.sum()]
    fdesc = rng.integers(0, 256, (nfr * cap, 32), dtype=np.uint8)
    fkps = np.zeros(nfr * cap, capi.KP_DTYPE)
    fkps["octave"] = rng.integers(0, 8, nfr * cap)
    owner = np.repeat(np.arange(m), nobs_p)
    fdesc[slot] = mp_desc[owner] ^ np.packbits(rng.random((len(slot), 256)) < 0.02, axis=1)
    ends = np.cumsum(nobs_p)
    lists = [((slot[e - c:e] // cap).astype(np.int32), (slot[e - c:e] % cap).astype(np.int32)) for e, c in zip(ends, nobs_p)]
    frames = mpt.DeviceFrames(fkps, fdesc, np.full(nfr, cap, np.int32), cap)
    batch = mpt.MainBatch(lists)
    batch.run(matcher, frames, None, False, nlevels=8)
    nm_c, idx_c = _projection_device(matcher, up(mp_pos), batch.out["main_desc"], batch.out["main_octave"], up(mp_skip), m, Tcw, K4,
                                     kps, desc, kf_obs)
    main = batch.download(matcher)
    ptr, fr, ft = mc.csr(lists)
    want = mm.update_main_batch(fkps, fdesc, np.full(nfr, cap, np.int32), cap, nfr, None, None, None, 8, ptr, fr, ft, None,
                                mc.sentinels(m))
    _same(main, want)
    nm_r, idx_r = matcher.MatchByProjection(mp_pos, main["main_desc"], main["main_octave"], mp_skip, Tcw, K4, kps, desc, kf_obs, 15, 2)
    assert nm_c == nm_r and np.array_equal(idx_c, idx_r) and nm_r > 50


def test_the_shared_observation_table(matcher):
    """the irregular table of tests/obs_table_cases.py, which the parallax and covisibility calls are fed too: planted entries
    out of range, a null frame, descending and overlapping d_mp_ptr segments (all inside 0..nobs)"""
    import obs_table_cases as oc
    from se2lam_amd import capi, mappoint as mpt
    t = oc.table()
    want = t.main_model(mm)
    assert (want["info"][[0, 10, 24], 0] == -1).all() and want["info"][9, 2] > want["info"][11, 2] > 0
    b = mpt.MainBatch([([e[0] for e in l], [e[1] for e in l]) for l in t.lists], t.prev, mc.sentinels(oc.M))
    assert b.nobs == t.nobs and 60 <= t.nobs <= 160 and b.m == oc.M
    b.mp_ptr = capi.upload(t.ptr)                          # the lists as they stand, the pointer array with its planted values
    b.run(matcher, mpt.DeviceFrames(t.kps, t.desc, oc.COUNTS, oc.CAP, t.frame_null, t.view), mc.SCALE)
    _same(b.download(matcher), want, "shared table")
