"""The one definition of the observation table (include/se2lam_amd/obs_table.h) through its three host mirrors at once:
MapPointMain.h, FindCorrespd.h and Covisibility.h run the table of tests/obs_table_cases.py and are held to their three numpy
models, which share no code with the header or with each other.  Integers exactly; floats as tests/test_mappoint_main_model.py
(to the bit), tests/test_new_kf_model.py (nc.same_parallax) and tests/test_covis_model.py (to the bit) compare them."""
import numpy as np
import pytest

import covis_cases as cc
import covis_model as cm
import mappoint_main_cases as mc
import mappoint_main_model as mm
import new_kf_cases as nc
import new_kf_model as nk
import obs_table_cases as oc


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("obs_table")
    return mc.cpp_build(d), nc.cpp_build(d), cc.cpp_build(d)


def test_the_table_holds_what_it_is_for():
    t = oc.table()
    f, k, seg = t.obs_frame, t.obs_ftr, t.segments()
    assert (f == -1).any() and (f == oc.NFRAMES).any() and (oc.COUNTS > oc.CAP).any()
    assert any(0 <= a < oc.NFRAMES and b == oc.COUNTS[a] < oc.CAP for a, b in zip(f, k))      # a feature at counts[f]
    assert any(0 <= a < oc.NFRAMES and b == oc.CAP for a, b in zip(f, k))                      # a feature at cap
    assert [p for p, (s, e) in enumerate(seg) if e < s] == [10, 24]
    inside = lambda a, b: seg[b][0] <= seg[a][0] and seg[a][1] <= seg[b][1] and seg[a][0] < seg[a][1]  # noqa: E731
    assert inside(11, 9) and inside(23, 25)
    assert 0 <= t.ptr.min() and t.ptr.max() <= t.nobs and 60 <= t.nobs <= 160
    assert sorted({len(l) for l in t.lists})[0] == 0 and max(e - s for s, e in seg) > 6


def test_one_table_through_the_three_host_mirrors(programs, tmp_path):
    t = oc.table()
    p_main, p_prl, p_covis = programs
    # MapPoint::updateMainKFandDescriptor, the null key frame 3 skipped
    want = t.main_model(mm)
    got = mc.cpp_run(p_main, tmp_path / "main.txt", oc.COUNTS, oc.CAP, mc.SCALE, t.kps["octave"], t.desc, t.frame_null, t.view, t.ptr,
                     t.obs_frame, t.obs_ftr, t.prev)
    mc.same(got, want)
    info = want["info"]
    assert (info[[0, 10, 24], 0] == -1).all() and info[9, 2] > info[11, 2] > 0 and info[25, 2] > info[23, 2] > 0
    s, e = t.segments()[1]
    assert info[1, 2] < e - s - 2                              # the planted entries and the null frame do not count
    # MapPoint::updateParallax, null key frames not skipped
    ref = t.parallax_model(nk.L32)
    assert np.array_equal(ref["status"], t.parallax_model(nk.L64)["status"]) and set(ref["status"]) == {0, 1, 2, 3}
    assert ref["status"][9] != 0 and ref["status"][25] != 0 and (ref["status"] == 1).sum() >= 4
    t.check_one_writer(ref["status"])
    _, got = nc.cpp_run_parallax(p_prl, tmp_path / "prl.txt", t.sc.fr, t.ptr, t.obs_frame, t.obs_ftr, t.good, t.new, t.observed)
    nc.same_parallax(got, ref)
    # Map::compareViewMPs, both overloads, every ordered pair of frames
    pa, pb = cc.pair_list(0, oc.NFRAMES)
    calls = [("pairs", int(a), int(b)) for a, b in zip(pa[:-4], pb[:-4])]
    calls += [("refset", kf, [r for r in range(-1, oc.NFRAMES + 1) if r != kf], k) for kf in range(oc.NFRAMES) for k in (1, 2, 3)]
    assert cc.against_header(p_covis, tmp_path / "covis.txt", [(t.covis_tables(), calls)]) == 36 + 18
    model = cm.Model(*cc.tables(t.covis_tables()))
    assert 9 in model.sets[oc.NEW] and (model.size_obs() > 0).all()
