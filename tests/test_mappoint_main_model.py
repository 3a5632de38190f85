"""MapPoint::updateMainKFandDescriptor without a device: the numpy model (tests/mappoint_main_model.py) against hand-worked
cases, and the host mirror include/se2lam_amd/MapPointMain.h (tests/cpp_mappoint_main.cpp) against the model, exactly."""
import numpy as np
import pytest

import mappoint_main_cases as mc
import mappoint_main_model as mm


def therm(t):
    """descriptor with the first t bits set: the distance of two of them is |t1 - t2|"""
    return np.packbits(np.arange(256) < t)


def test_one_observation_is_its_own_main():
    assert mm.main_of(np.stack([therm(17)])) == (0, 0)


def test_two_observations_always_tie_and_the_first_wins():
    # rows [0, 5] and [0, 5]: element (2 - 1) // 2 = 0 of both is the self-distance 0
    assert mm.main_of(np.stack([therm(9), therm(4)])) == (0, 0)
    assert mm.main_of(np.stack([therm(4), therm(9)])) == (0, 0)


def test_three_observations_planted_tie_goes_to_the_earlier():
    A, B = therm(0), therm(3)
    X = np.packbits((np.arange(256) >= 100) & (np.arange(256) < 200))      # 100 bits away from A, 103 from B
    assert mm.distance_table(np.stack([X, A, B])).tolist() == [[0, 100, 103], [100, 0, 3], [103, 3, 0]]
    # medians (element 1): X 100, A 3, B 3 -> A and B tie, the earlier one in the list wins
    assert mm.main_of(np.stack([X, A, B])) == (1, 3)
    assert mm.main_of(np.stack([X, B, A])) == (1, 3)
    assert mm.main_of(np.stack([B, A, X])) == (0, 3)


def test_four_observations_take_the_lower_middle():
    # t = 0, 10, 11, 13: sorted rows [0 10 11 13] [0 1 3 10] [0 1 2 11] [0 2 3 13].  Element (4 - 1) // 2 = 1: medians
    # 10, 1, 1, 2 -> place 1 (first of the tie).  The upper middle (element 2: 11, 3, 2, 3) would pick place 2.
    assert mm.main_of(np.stack([therm(t) for t in (0, 10, 11, 13)])) == (1, 1)


def test_distances_are_float32_of_the_float64_norm():
    mn, mx = mm.min_max_dist(np.array([3, 4, 12], np.float32), 2, mc.SCALE)
    assert mx == np.float32(13.0) * mc.SCALE[2] and mn == np.float32(mx / mc.SCALE[-1])
    assert mn.dtype == np.float32 and mx.dtype == np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return mc.cpp_build(tmp_path_factory.mktemp("mappoint_main"))


def _run_mirror(program, tmp_path, fs, kps, null, view, lists, prev):
    return mc.cpp_run(program, tmp_path / "case.txt", fs.counts, mc.CAP, mc.SCALE, kps["octave"], fs.desc, null,
                      fs.view if view else None, *mc.csr(lists), prev)


_same = mc.same


def test_host_mirror_equals_the_model(program, tmp_path):
    fs = mc.FrameSet()
    lists = mc.first_batch(fs)
    rng = np.random.default_rng(3)
    null = (rng.random(mc.NFRAMES) < 0.1).astype(np.uint8)
    # observations to skip: frames -1 and nframes, features at counts and at cap
    f, k = lists[8]
    lists[8] = (np.concatenate([[-1, mc.NFRAMES, 2, 0], f]).astype(np.int32), np.concatenate([[0, 0, 10, mc.CAP], k]).astype(np.int32))
    m = len(lists)
    args = fs.model_args(null=null)
    ptr, fr, ft = mc.csr(lists)
    want = mm.update_main_batch(mp_ptr=ptr, obs_frame=fr, obs_ftr=ft, prev_main_frame=None, out=mc.sentinels(m), **args)
    _same(_run_mirror(program, tmp_path, fs, fs.kps, null, True, lists, None), want)
    assert (want["info"][:, 0] == -1).sum() >= 1 and (want["info"][:, 2] > 64).sum() >= 2

    # the previous main frame equal to the winner for every other point; an octave outside the scale factors
    prev = np.where(np.arange(m) % 2 == 0, want["main_frame"], 3).astype(np.int32)
    kps = fs.kps.copy()
    q = next(p for p in range(1, m, 2) if want["info"][p, 0] >= 0 and want["main_frame"][p] != 3)
    e = next(p for p in range(0, m, 2) if want["info"][p, 0] >= 0)
    off = int(want["main_frame"][q]) * mc.CAP + int(ft[ptr[q] + want["info"][q, 0]])
    kps["octave"][off] = mc.NLEVELS
    args["kps"] = kps
    want2 = mm.update_main_batch(mp_ptr=ptr, obs_frame=fr, obs_ftr=ft, prev_main_frame=prev, out=mc.sentinels(m), **args)
    assert want2["info"][q, 3] == 3 and want2["main_octave"][e] == -77 and want2["info"][e, 3] == 0
    _same(_run_mirror(program, tmp_path, fs, kps, null, True, lists, prev), want2)
    # without view positions no distance is written
    args["view_pos"] = None
    want3 = mm.update_main_batch(mp_ptr=ptr, obs_frame=fr, obs_ftr=ft, prev_main_frame=prev, out=mc.sentinels(m), **args)
    assert (want3["dist"] == -1.0).all()
    _same(_run_mirror(program, tmp_path, fs, kps, null, False, lists, prev), want3)
