"""tests/feat_edge_gather_model.py (the numpy statement of se2gpu_feat_edge_batch_device's two gathers) on hand cases whose answers
are written down here, and the host function se2gpu_plane_motion_prior_iso3 against its own recorded outputs
(tests/golden/plane_prior_iso3.npz, tools/gen_plane_prior_golden.py): its arithmetic is shared with the device kernel and must
not move by a bit.  No device."""
import os

import numpy as np
import pytest

import feat_edge_gather_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NF, M, NOBS = 3, 6, 8


def _tables():
    Twc = np.arange(NF * 12, dtype=np.float32).reshape(NF, 12) + 0.5
    pos = (100 + np.arange(M * 3, dtype=np.float32)).reshape(M, 3)
    view = (200 + np.arange(NOBS * 3, dtype=np.float32)).reshape(NOBS, 3)
    info = (300 + np.arange(NOBS * 9, dtype=np.float32)).reshape(NOBS, 9)
    return Twc, pos, view, info


def test_pose_rows_become_rotation_and_translation():
    Twc = _tables()[0]
    k = gm.kf12_of_slot(Twc, 1, NF)
    row = Twc[1].astype(np.float64)                      # r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz
    assert k.tolist() == [row[0], row[1], row[2], row[4], row[5], row[6], row[8], row[9], row[10], row[3], row[7], row[11]]
    assert k.dtype == np.float64
    for slot in (-1, NF):
        assert gm.kf12_of_slot(Twc, slot, NF).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def _covis(pair_out, common, list_cap, row_cap, pair_a=(0,), pair_b=(1,)):
    Twc, pos, view, info = _tables()
    return gm.gather_covis(list(pair_a), list(pair_b), NF, Twc, pos, row_cap, np.array(pair_out, np.int32), np.array(common, np.int32),
                           list_cap, view, info), (pos, view, info)


def test_covis_an_invalid_entry_in_the_middle_is_dropped_and_the_rest_closes_up():
    common = [[(0, 0, 1), (1, 2, -1), (2, 3, 4), (5, 7, 6)]]
    for bad in ((1, 2, -1), (1, NOBS, 3), (M, 2, 3), (-1, 2, 3), (1, -5, 3)):
        common[0][1] = bad
        g, (pos, view, info) = _covis([[4, 9, 9, 0]], common, 4, 8)
        assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (3, 4, 1, 0)
        assert np.array_equal(g["xyz"][0], pos[[0, 2, 5]].astype(np.float64))
        assert np.array_equal(g["z"][0], np.hstack([view[[0, 3, 7]], view[[1, 4, 6]]]).astype(np.float64))
        assert np.array_equal(g["info"][0], np.hstack([info[[0, 3, 7]], info[[1, 4, 6]]]).astype(np.float64))


@pytest.mark.parametrize("n_same,want", [(-1, (0, -1, 0, 0)), (0, (0, 0, 0, 0)), (3, (3, 3, 0, 0)), (4, (3, 4, 0, 1))])
def test_covis_n_same_against_list_cap(n_same, want):
    """list_cap = 3: n_same = -1 (a slot the pairs call refused), 0, list_cap, list_cap + 1; entries past the list are never read"""
    common = [[(0, 0, 1), (1, 2, 3), (2, 4, 5)]]
    g, _ = _covis([[n_same, 0, 0, 0]], common, 3, 8)
    assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == want
    assert len(g["xyz"][0]) == want[0]


def test_covis_row_cap_cuts_before_validity_and_bad_slots_give_no_points():
    common = [[(0, 0, 1), (9, 2, 3), (2, 4, 5), (3, 6, 7)]] * 3
    g, (pos, _, _) = _covis([[4, 0, 0, 0]] * 3, common, 4, 2, pair_a=(0, -1, 0), pair_b=(1, 1, NF))
    # the first row_cap = 2 entries are taken, the second of them is invalid
    assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (1, 4, 1, 1)
    assert np.array_equal(g["xyz"][0], pos[[0]].astype(np.float64))
    for p in (1, 2):
        assert (g["count"][p], g["raw"][p], g["dropped"][p], g["cut"][p]) == (0, 4, 0, 0)
    assert g["kf12"][1, 0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and g["kf12"][2, 1].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(g["kf12"][1, 1], gm.kf12_of_slot(_tables()[0], 1, NF))


CAP = 6


def _match(row, counts, ftr_mp, row_cap, a=0, b=1):
    Twc, pos, _, _ = _tables()
    vpos = (400 + np.arange(NF * CAP * 3, dtype=np.float32)).reshape(NF, CAP, 3)
    vinfo = (500 + np.arange(NF * CAP * 9, dtype=np.float32)).reshape(NF, CAP, 9)
    g = gm.gather_match([a], [b], NF, Twc, pos, row_cap, np.array([row], np.int32), np.array(counts, np.int32), CAP,
                        np.array(ftr_mp, np.int32), vpos, vinfo)
    return g, pos, vpos, vinfo


def test_match_row_rules():
    """-1, a value past counts[b], an entry past counts[a], no map point on either side, a point index past m"""
    ftr = [[0, 1, -1, 3, 4, 5],          # frame a: feature 2 has no point
           [5, 4, -1, M, 1, 0],          # frame b: feature 2 has none; feature 3 names a point past m (only >= 0 is asked of b)
           [0] * CAP]
    row = [4, -1, 0, 2, 3, 1]            # i=0 -> 4 ok; i=1 none; i=2 -> 0 but a has no point; i=3 -> 2, b has none; i=4 -> 3 ok; i=5 past counts[a]
    g, pos, vpos, vinfo = _match(row, [5, 5, 0], ftr, 8)
    assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (2, 4, 2, 0)
    assert np.array_equal(g["xyz"][0], pos[[0, 4]].astype(np.float64))
    assert np.array_equal(g["z"][0], np.hstack([vpos[0, [0, 4]], vpos[1, [4, 3]]]).astype(np.float64))
    assert np.array_equal(g["info"][0], np.hstack([vinfo[0, [0, 4]], vinfo[1, [4, 3]]]).astype(np.float64))
    # j >= counts[b] is no raw match
    g, *_ = _match(row, [5, 4, 0], ftr, 8)
    assert (g["count"][0], g["raw"][0], g["dropped"][0]) == (1, 3, 2)
    # a point index of frame a past m is no point; counts beyond cap are clamped
    ftr2 = [list(r) for r in ftr]
    ftr2[0][0] = M
    g, *_ = _match(row, [99, 99, 0], ftr2, 8)
    assert (g["count"][0], g["raw"][0], g["dropped"][0]) == (2, 5, 3)       # i=5 -> 1 joins: (a,5) = 5, (b,1) = 4
    assert np.array_equal(g["xyz"][0], pos[[4, 5]].astype(np.float64))


def test_match_row_cap_cuts_the_points_and_not_the_raw_count():
    ftr = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0] * CAP]
    g, pos, *_ = _match([0, 1, 2, 3, 4, 5], [6, 6, 0], ftr, 4)
    assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (4, 6, 0, 1)
    assert np.array_equal(g["xyz"][0], pos[:4].astype(np.float64))
    g, *_ = _match([0, 1, 2, 3, 4, 5], [6, 6, 0], ftr, 6)
    assert (g["count"][0], g["cut"][0]) == (6, 0)
    for a, b in ((-1, 1), (0, NF)):
        g, *_ = _match([0, 1, 2, 3, 4, 5], [6, 6, 0], ftr, 4, a=a, b=b)
        assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (0, 0, 0, 0)


def test_host_call_arrays_are_the_csr_of_the_counts():
    common = [[(0, 0, 1), (9, 2, 3), (2, 4, 5)], [(1, 1, 1), (2, 2, 2), (3, 3, 3)]]
    g, _ = _covis([[3, 0, 0, 0], [3, 0, 0, 0]], common, 3, 8, pair_a=(0, 1), pair_b=(1, 2))
    kf, mp_ptr, mp, z, info = gm.host_call_arrays(g)
    assert mp_ptr.tolist() == [0, 2, 5] and mp.shape == (5, 3) and z.shape == (5, 6) and info.shape == (5, 18) and kf.shape == (2, 2, 12)


def test_plane_motion_prior_host_function_keeps_its_recorded_bits():
    from se2lam_amd import capi
    g = np.load(os.path.join(ROOT, "tests", "golden", "plane_prior_iso3.npz"))
    Twc12, tbc, (xrot, yrot, zinfo) = np.ascontiguousarray(g["Twc12"]), np.ascontiguousarray(g["Tbc12"]), g["infos"]
    assert Twc12.shape == (100, 12)
    meas, info = np.zeros((100, 12)), np.zeros((100, 36))
    for i in range(100):
        capi.check(capi.lib().se2gpu_plane_motion_prior_iso3(Twc12[i].ctypes.data, tbc.ctypes.data, float(xrot), float(yrot), float(zinfo),
                                                             meas[i].ctypes.data, info[i].ctypes.data))
    assert np.array_equal(meas.view(np.uint64), g["meas12"].view(np.uint64))
    assert np.array_equal(info.view(np.uint64), g["info36"].view(np.uint64))
    # the poses exercise what the formula is about: roll and pitch are removed, so the measurement differs from the input
    assert np.abs(meas - Twc12).max() > 1e-3
