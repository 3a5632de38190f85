"""tests/map_apply_model.py on hand-stated cases, one per rule of se2gpu_map_apply_batch_device (include/se2gpu.h), and on the
reference's own map: tests/golden/map_apply_ref.npz holds the observation lists of the reference's CPU pipeline after every new
key frame of a 120-frame run (tools/gen_map_apply_golden.py), 11 transitions of which 7 prune a key frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_apply_cases as mc   # noqa: E402
import map_apply_golden as mg  # noqa: E402
import map_apply_model as mm   # noqa: E402

f32 = np.float32
S = mm


def lists(out):
    m = out["sizes_out"][S.M_NEW]
    return mm.lists_of(out["mp_ptr_new"], out["obs_frame_new"], out["obs_ftr_new"], m)


def test_kind1_appends_to_the_point_the_previous_key_frame_holds():
    c = mc.kind1_alone()
    o = mm.apply(c)
    assert lists(o) == [[(0, 1), (1, 2), (3, 0)], [(1, 3), (3, 4)], [(0, 5), (1, 5), (2, 5)], [(2, 7)]]
    assert o["sizes_out"].tolist() == [0, 4, 9, 2, 0, 0, 0, 0, 0] and o["job_counts"].tolist() == [[0, 2, 0, 0, 0, 0]]
    assert o["ftr_mp"][3 * 16 + 0] == 0 and o["ftr_mp"][3 * 16 + 4] == 1 and o["kf_observed"][3 * 16 + 4] == 1
    assert o["new_frame"][:5].tolist() == [3, 3, -1, -1, -1]
    assert np.array_equal(o["view_pos"][3 * 16 + 4], c["view"][0, 4]) and np.array_equal(o["obs_info_new"][4], c["info"][0, 4])
    # mNormalVector = (n * 2 + unit(view)) / 3 in float, the unit vector through doubles
    v = c["view"][0, 0].astype(np.float64)
    u = (v / np.sqrt((v * v).sum())).astype(f32)
    want = ((c["mp_normal"][0] * f32(2) + u) * (f32(1) / f32(3))).astype(f32)
    assert np.array_equal(o["mp_normal"][0], want)
    assert np.array_equal(o["obs_view_new"][:2], c["obs_view"][:2])      # the kept rows travel with their entries


def test_kind2_appends_to_the_named_point():
    o = mm.apply(mc.kind2_alone())
    assert lists(o)[3] == [(2, 7), (3, 2)] and o["ftr_mp"][3 * 16 + 2] == 3
    assert o["job_counts"].tolist() == [[0, 0, 1, 0, 0, 0]]


def test_kind3_slots_follow_src_not_j():
    c = mc.kind3_alone()
    o = mm.apply(c)
    assert lists(o)[4:] == [[(1, 4), (3, 5)], [(1, 6), (3, 7)], [(1, 9), (3, 1)]]
    assert o["sizes_out"].tolist() == [0, 7, 13, 6, 0, 3, 0, 0, 0]
    assert o["good_prl"][4:7].tolist() == [1, 1, 0] and o["mp_null"][4:8].tolist() == [0, 0, 0, 1]
    assert np.array_equal(o["pos"][6], c["new_pos_w"][0, 1]) and o["ftr_mp"][1 * 16 + 9] == 6 and o["ftr_mp"][3 * 16 + 1] == 6
    assert np.array_equal(o["view_pos"][1 * 16 + 9], c["local_pos"][0, 9]) and np.array_equal(o["view_info"][1 * 16 + 9], c["info_prev"][0, 1])
    assert np.array_equal(o["obs_view_new"][11], c["local_pos"][0, 9]) and np.array_equal(o["obs_info_new"][12], c["info"][0, 1])
    n = mm.normal_add(mm.normal_add(np.zeros(3, f32), c["local_pos"][0, 9], 0), c["view"][0, 1], 1)
    assert np.array_equal(o["mp_normal"][6], n) and abs(np.linalg.norm(n) - 1) < 0.3


def test_mixed_and_the_kinds_mask():
    o = mm.apply(mc.mixed())
    assert o["job_counts"].tolist() == [[0, 1, 1, 2, 0, 0]] and o["sizes_out"][S.M_NEW] == 6
    assert lists(o)[4:] == [[(1, 8), (3, 9)], [(1, 11), (3, 3)]]
    o1 = mm.apply(mc.mixed(2))
    assert o1["job_counts"].tolist() == [[0, 1, 0, 0, 0, 0]] and o1["sizes_out"][S.M_NEW] == 4
    o2 = mm.apply(mc.mixed(12))
    assert o2["job_counts"].tolist() == [[0, 0, 1, 2, 0, 0]] and lists(o2)[0] == [(0, 1), (1, 2)]


def test_two_jobs_append_in_job_order():
    o = mm.apply(mc.two_jobs_one_point())
    assert lists(o)[3] == [(2, 7), (3, 6), (4, 2), (5, 9)]
    assert o["new_frame"][3] == 5
    assert lists(o)[4:] == [[(1, 10), (3, 8)], [(0, 12), (4, 4)]]        # job 0's point before job 1's


def test_duplicate_claims_the_greatest_j_wins():
    o = mm.apply(mc.duplicate_claim())
    assert lists(o)[3] == [(2, 7), (3, 6)] and lists(o)[4] == [(1, 9), (3, 8)]
    assert o["sizes_out"][S.SKIPPED] == 2 and o["sizes_out"][S.DUP] == 2 and o["job_counts"].tolist() == [[0, 0, 1, 1, 2, 2]]
    assert o["kf_observed"][3 * 16 + 2] == 0 and o["ftr_mp"][3 * 16 + 2] == -1


def test_refused_targets_are_skipped_and_their_flags_cleared():
    c = mc.refused_targets()
    o = mm.apply(c)
    assert o["job_counts"].tolist() == [[0, 0, 1, 0, 6, 0]]
    assert o["kf_observed"][3 * 16:3 * 16 + 8].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert (o["ftr_mp"][3 * 16:3 * 16 + 7] == -1).all() and np.array_equal(o["view_pos"][3 * 16:3 * 16 + 7], c["view_pos"][3 * 16:3 * 16 + 7])
    assert lists(o)[1] == [] and o["ftr_mp"][1 * 16 + 3] == -1           # the null point's own entry went in rule 1


def test_a_point_the_frame_already_observes_keeps_its_entry():
    o = mm.apply(mc.already_observed())
    assert lists(o)[0] == [(0, 1), (1, 2)] and lists(o)[3] == [(2, 7), (1, 10)]
    assert o["ftr_mp"][1 * 16 + 2] == 0 and o["kf_observed"][1 * 16 + 9] == 0 and o["sizes_out"][S.SKIPPED] == 1


def test_a_null_frame_is_erased_and_empty_points_become_null():
    c = mc.erase_null_frame()
    o = mm.apply(c)
    assert lists(o) == [[(0, 1)], [], [(0, 5), (2, 5)], [(2, 7)], [], [(2, 10)]]
    assert o["mp_null"][:6].tolist() == [0, 1, 0, 0, 1, 0] and o["good_prl"][1] == 0
    assert (o["ftr_mp"][16:32] == -1).all() and not o["kf_observed"][16:32].any()
    assert o["sizes_out"].tolist() == [0, 6, 5, 0, 6, 0, 2, 0, 0]
    n = mm.normal_erase(c["mp_normal"][5], c["view_pos"][1 * 16 + 10], 2)  # in list order: (1, 10), then (1, 11)
    n = mm.normal_erase(n, c["view_pos"][1 * 16 + 11], 1)
    assert np.array_equal(o["mp_normal"][5], n)
    assert np.array_equal(o["mp_normal"][1], c["mp_normal"][1])            # setNull leaves the vector
    o2 = mm.apply(mc.erase_null_frame_and_add())
    assert o2["job_counts"].tolist() == [[0, 0, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0]]
    assert lists(o2)[5] == [(2, 10), (4, 4)] and lists(o2)[6] == [(2, 2), (4, 6)] and lists(o2)[1] == []


def test_null_points_and_abandoned_points_lose_their_entries():
    c = mc.erase_null_point_and_status()
    o = mm.apply(c)
    assert lists(o) == [[], [(1, 3)], [], [(2, 7)]]
    assert o["mp_null"][:4].tolist() == [1, 0, 1, 0] and o["good_prl"][:4].tolist() == [0, 1, 0, 1]
    assert o["ftr_mp"][[1, 16 + 2, 5, 16 + 5, 32 + 5]].tolist() == [-1] * 5 and o["ftr_mp"][16 + 3] == 1
    assert o["sizes_out"][S.ERASED] == 5 and o["sizes_out"][S.NULLED] == 1


def test_an_invalid_old_entry_is_dropped_without_a_trace():
    c = mc.invalid_old_entry()
    o = mm.apply(c)
    assert lists(o) == [[(0, 1), (1, 2), (3, 1)], [], [(0, 5), (1, 5), (2, 5)], []]
    assert o["mp_null"][:4].tolist() == [0, 1, 0, 1]
    assert np.array_equal(o["mp_normal"][0], mm.normal_add(c["mp_normal"][0], c["view"][0, 1], 2))   # oldObsSize counts valid entries


def test_a_list_of_more_than_64_entries():
    c = mc.long_list()
    o = mm.apply(c)
    got = lists(o)
    assert len(got[1]) == 70 - 14 + 1 and got[1][-1] == (5, 3) and got[1][:3] == [(1, 0), (2, 0), (3, 0)]
    assert o["job_counts"].tolist() == [[0, 1, 1, 0, 0, 0]] and got[2] == [(2, 14), (5, 4)]
    assert np.isfinite(o["mp_normal"][1]).all() and not np.array_equal(o["mp_normal"][1], c["mp_normal"][1])


@pytest.mark.parametrize("name,need", [("capacity_points", (6, 12)), ("capacity_entries", (5, 10))])
def test_capacity_status_modifies_nothing(name, need):
    c = mc.CASES[name]()
    o = mm.apply(c)
    assert o["sizes_out"][S.STATUS] == 2 and (o["sizes_out"][S.M_NEW], o["sizes_out"][S.NOBS_NEW]) == need
    for k in mm.INPLACE:
        assert np.array_equal(o[k], c[k]), k


def test_padding_and_bad_jobs():
    c = mc.bad_jobs()
    o = mm.apply(c)
    assert o["job_counts"][:, 0].tolist() == [1, 1, 1, 0] and o["job_counts"][3].tolist() == [0, 0, 1, 0, 0, 0]
    m, n = o["sizes_out"][S.M_NEW], o["sizes_out"][S.NOBS_NEW]
    assert (o["mp_ptr_new"][m:] == n).all() and len(o["mp_ptr_new"]) == c["m_cap"] + 1
    assert o["mp_null"][m:].all() and not o["good_prl"][m:].any() and (o["new_frame"][m:] == -1).all()
    assert (o["obs_frame_new"][n:] == mm.ISENT).all()
    # the padded table read with m = m_cap, nobs = nobs_cap by the segment rule is the exact-size table
    assert mm.lists_of(o["mp_ptr_new"], o["obs_frame_new"], o["obs_ftr_new"], c["m_cap"])[m:] == [[]] * (c["m_cap"] - m)


def test_calls_follow_one_another_and_random_tables_stay_consistent():
    for name in ("random_small", "random_scan"):
        c = mc.CASES[name]()
        o = mm.apply(c)
        assert o["sizes_out"][S.STATUS] == 0 and o["sizes_out"][S.CREATED] > 0 and o["sizes_out"][S.SKIPPED] > 0
        assert o["sizes_out"][S.ERASED] > 0 and o["sizes_out"][S.NULLED] > 0
        o2 = mm.apply(mm.next_case(c, o))                                 # nothing left to do: the same table again
        assert lists(o2) == lists(o) and o2["sizes_out"][S.ADDED] == 0
        for k in mm.INPLACE:
            assert np.array_equal(o2[k], o[k]), k


def test_the_reference_map_all_eleven_transitions():
    g = mg.Golden()
    assert g.ntransitions == 11 and sum(t["pruned"] is not None for t in g.transitions) == 7
    c = g.first_case()
    done = 0
    for t in g.transitions:
        assert 635 <= t["n_new_entries"] <= 736 and 89 <= t["n_created"] <= 140 or t["index"] == 0
        c = g.add_case(c, t)
        o = mm.apply(c)
        assert o["sizes_out"][S.STATUS] == 0 and o["sizes_out"][S.SKIPPED] == 0 and o["sizes_out"][S.DUP] == 0
        assert o["sizes_out"][S.CREATED] == t["n_created"]
        c = g.erase_case(c, o, t)
        o = mm.apply(c)
        if t["pruned"] is not None:
            assert 775 <= o["sizes_out"][S.ERASED] <= 825
        g.check_state(o, t)                                               # entry sets, n_obs, which points exist, slots by mId
        c = mm.next_case(c, o)
        done += 1
    assert done == 11                                                     # the share of transitions left out is zero
