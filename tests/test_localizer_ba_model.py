"""tests/localizer_ba_model.py, the numpy statement the GPU test of se2gpu_localizer_ba_batch_device compares against, checked on
the CPU: against the compiled reference's Localizer::DoLocalBA (oracle/_ref), against the restatement of the plane-motion prior
(oracle), on hand-stated maps for every rule, and - before a case ships to the GPU test - that the restatement's LM has something
to compare on it."""
import numpy as np
import pytest

import localizer_ba_cases as cases
import localizer_ba_model as model
from oracle import ref
from test_pose_ba import CX, CY, DELTA, F, TBC, _Twb


def _single_frame(Tcw0, Xw, kps, good):
    n = len(Xw)
    return dict(Tcw=Tcw0[:3, :4].reshape(1, 12).astype(np.float32), kps_xy=np.stack([kps["x"], kps["y"]], 1)[None].astype(np.float32),
                kps_octave=kps["octave"][None].astype(np.int32), counts=np.array([n], np.int32), ftr_mp=np.arange(n, dtype=np.int32)[None],
                kf_observed=np.ones((1, n), np.uint8), pos=Xw.astype(np.float32), mp_null=np.zeros(n, np.uint8), good_prl=good,
                inv_level_sigma2=cases.inv_level_sigma2(), Tbc12=cases.tbc12(), xrot_info=1e6, yrot_info=1e6, z_info=1.0)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built and the reference's sources are not here")
@pytest.mark.parametrize("seed,n", [(0, 400), (2, 37), (4, 6)])
def test_model_against_the_compiled_reference(oracle, seed, n):
    """the three cases of test_do_local_ba_of_the_compiled_reference: the graph Localizer::DoLocalBA built, as compiled"""
    from test_ref_compiled import _pose_only_case
    Tcw0, Xw, kps, tbc, f, cx, cy, delta = _pose_only_case(seed, n)
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32)
    good = np.ones(n, np.uint8); good[::9] = 0
    out = ref.localizer_do_local_ba(K, tbc, np.float32(delta), Tcw0, kps, Xw, good)
    got = model.job(_single_frame(Tcw0, Xw, kps, good), 0, None, -1)
    order = np.argsort(out["e_point"])                                  # the reference walks a std::set of pointers
    assert np.array_equal(out["e_point"][order], got["e_ftr"])         # point i is feature i here
    assert np.array_equal(out["e_uv"][order], got["uv"]) and np.array_equal(out["e_w"][order], got["w"])
    assert tuple(got["info"][:3]) == (n, n, int(good.sum()))
    assert np.allclose(out["prior_meas"], cases.matrix(got["prior_meas"]), rtol=0, atol=1e-9)
    assert np.allclose(out["prior_info"], got["prior_info"], rtol=1e-9, atol=1e-9 * np.abs(got["prior_info"]).max())
    _, st = oracle.pose_only_ba(cases.matrix(got["pose0"]), cases.matrix(got["prior_meas"]), got["prior_info"], got["xyz"], got["uv"], got["w"],
                                float(K[0, 0]), float(K[0, 2]), float(K[1, 2]), float(np.float32(delta)), 30)
    assert np.isclose(out["chi2"], st["chi2_init"], rtol=1e-9, atol=0)


def test_model_prior_against_the_restatement(oracle):
    """the tolerances of test_plane_motion_prior_matches_restatement"""
    poses = [np.linalg.inv(_Twb(300, -200, 0.7) @ TBC), np.linalg.inv(_Twb(-900, 50, -2.9, roll=0.03, z=20) @ TBC)]
    T = cases.tables()
    poses += [cases.matrix(model.pose12(model.start_pose(T["Tcw"][f]))) for f in range(cases.NFRAMES)]
    for P in poses:
        meas, info = model.plane_motion_prior((P[:3, :3], P[:3, 3]), (TBC[:3, :3], TBC[:3, 3]), 1e6, 1e6, 1.0)
        mo, io = oracle.plane_motion_prior(P, TBC)
        assert np.allclose(cases.matrix(model.pose12(meas)), mo, rtol=0, atol=1e-12)
        assert np.allclose(info, io, rtol=1e-13, atol=0)


def test_start_pose_is_a_rotation_close_to_the_floats():
    T = cases.tables()
    for f in range(cases.NFRAMES):
        R, t = model.start_pose(T["Tcw"][f])
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
        assert np.allclose(R, T["Tcw"][f].reshape(3, 4)[:, :3], atol=2e-7) and np.array_equal(t, T["Tcw"][f].reshape(3, 4)[:, 3].astype(np.float64))


def _hand(ftr_mp, counts=None, m=6, null=(), bad=(), octave=None):
    """one frame of cap = 8 features over m points, every number easy to see"""
    cap = 8
    row = np.full(cap, -1, np.int32); row[:len(ftr_mp)] = ftr_mp
    mp_null, good = np.zeros(m, np.uint8), np.ones(m, np.uint8)
    mp_null[list(null)] = 1; good[list(bad)] = 0
    oc = np.zeros(cap, np.int32) if octave is None else np.asarray(octave, np.int32)
    Tcw = np.linalg.inv(_Twb(100, 50, 0.3) @ TBC)[:3, :4].reshape(1, 12).astype(np.float32)
    return dict(Tcw=Tcw, kps_xy=(10.0 * np.arange(2 * cap, dtype=np.float32)).reshape(1, cap, 2), kps_octave=oc[None],
                counts=np.array([cap if counts is None else counts], np.int32), ftr_mp=row[None], kf_observed=(row[None] >= 0).astype(np.uint8),
                pos=(100.0 * np.arange(3 * m, dtype=np.float32)).reshape(m, 3), mp_null=mp_null, good_prl=good,
                inv_level_sigma2=cases.inv_level_sigma2(), Tbc12=cases.tbc12(), xrot_info=1e6, yrot_info=1e6, z_info=1.0)


def test_hand_stated_rules():
    # renewal: feature 1 takes point 4; the null point 5 leaves feature 2 as it was; -1 and indices past the table do nothing
    T = _hand([0, -1, 2, -1], null=(5,))
    g = model.job(T, 0, np.array([-1, 4, 5, 99, -3, -1, -1, -1]), -1)
    assert g["ftr_mp"].tolist() == [0, 4, 2, -1, -1, -1, -1, -1] and g["kf_observed"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert g["info"].tolist() == [8, 3, 3, 1, 0, 0, 0, 0] and g["e_ftr"].tolist() == [0, 1, 2]
    assert np.array_equal(g["xyz"][1], T["pos"][4].astype(np.float64)) and np.array_equal(g["uv"][1], [20.0, 30.0])
    # a duplicate: point 3 under features 0 and 5 counts once and keeps feature 5; the edges stay in ascending feature order
    g = model.job(_hand([3, 1, -1, -1, -1, 3]), 0, None, -1)
    assert g["info"].tolist() == [8, 2, 2, 0, 1, 0, 0, 0] and g["e_ftr"].tolist() == [1, 5]
    # a renewal makes the duplicate: the match row hands point 0 (held by feature 0) to feature 6
    g = model.job(_hand([0, 1]), 0, np.array([-1, -1, -1, -1, -1, -1, 0, -1]), -1)
    assert g["info"].tolist() == [8, 2, 2, 1, 1, 0, 0, 0] and g["e_ftr"].tolist() == [1, 6]
    # an entry outside -1..m-1 is skipped and flagged; null and bad-parallax points count as observations and give no edge
    g = model.job(_hand([0, 6, -2, 4, 5, 1], null=(4,), bad=(5,)), 0, None, -1)
    assert g["info"].tolist() == [8, 4, 2, 0, 0, model.FLAG_ENTRY, 0, 0] and g["e_ftr"].tolist() == [0, 5]
    # an octave outside the levels drops the edge and is flagged; the weight is the feature's own octave's
    g = model.job(_hand([0, 1, 2], octave=[3, 8, -1, 0, 0, 0, 0, 0]), 0, None, -1)
    assert g["info"].tolist() == [8, 3, 1, 0, 0, model.FLAG_OCTAVE, 0, 0] and g["w"].tolist() == [float(cases.inv_level_sigma2()[3])]
    # features past counts are not read; a slot outside the table is status 1
    g = model.job(_hand([0, 1, 2, 3], counts=2), 0, np.array([-1, -1, 4, -1, -1, -1, -1, -1]), -1)
    assert g["info"].tolist() == [2, 2, 2, 0, 0, 0, 0, 0] and g["ftr_mp"][2] == 2
    assert model.job(_hand([0]), 1, None, -1)["status"] == 1 and model.job(_hand([0]), -1, None, -1)["status"] == 1


def test_the_gate_at_30_and_31():
    """numMPCurr > 30 (Localizer.cpp:95): 30 distinct points do not run, 31 do; null and bad-parallax points count"""
    T = cases.tables(edges=(26, 27, 30, 31, 0, 0))        # frames 0, 1: + 2 null + 2 bad parallax = 30, 31 observations
    assert [model.job(T, f, None, 30)["status"] for f in range(4)] == [5, None, None, None]
    assert [int(model.job(T, f, None, 30)["info"][1]) for f in range(4)] == [30, 31, 34, 35]
    assert [int(model.job(T, f, None, 30)["info"][2]) for f in range(4)] == [26, 27, 30, 31]
    T = cases.tables(edges=(30, 31, 0, 0, 0, 0))
    T["ftr_mp"][:2][T["ftr_mp"][:2] >= cases.GOOD] = -1   # without the four: 30 and 31 good points
    assert [model.job(T, f, None, 30)["status"] for f in range(2)] == [5, None]
    assert model.job(T, 0, None, -1)["status"] is None and model.job(T, 0, None, 29)["status"] is None


def _history_cases():
    T, R = cases.tables(), cases.tables(shift_uv=cases.REJECT)
    return [(T, f) for f in cases.HISTORY_FRAMES] + [(R, cases.REJECT[0])]


def test_shipped_cases_have_a_history_to_compare(oracle):
    """_same_run needs two iterations whose cost still drops by more than 1e-9 relative; the outlier start must reject trials"""
    rows = cases.match_rows(cases.tables(), list(cases.HISTORY_FRAMES))
    for i, (T, f) in enumerate(_history_cases()):
        for match in (None, rows[i] if i < len(cases.HISTORY_FRAMES) else None):
            g = model.job(T, f, match, -1)
            assert len(g["e_ftr"]) >= 6
            _, st = oracle.pose_only_ba(cases.matrix(g["pose0"]), cases.matrix(g["prior_meas"]), g["prior_info"], g["xyz"], g["uv"], g["w"],
                                        F, CX, CY, DELTA, 30)
            assert cases.live_iterations(st) >= 2, (f, st["chi2_init"], st["chi2_hist"])
    T, f = _history_cases()[-1]
    g = model.job(T, f, None, -1)
    _, st = oracle.pose_only_ba(cases.matrix(g["pose0"]), cases.matrix(g["prior_meas"]), g["prior_info"], g["xyz"], g["uv"], g["w"], F, CX, CY, DELTA, 30)
    assert max(st["trials_hist"]) > 1, st["trials_hist"]


def test_match_rows_exercise_every_renewal_rule():
    T = cases.tables()
    frames = [1, 2, 3, 4, 5]
    rows = cases.match_rows(T, frames)
    for b, f in enumerate(frames):
        g = model.job(T, f, rows[b], -1)
        assert g["info"][3] >= 3 and g["info"][4] >= 1, (f, g["info"])       # renewed, duplicates
        n = int(T["counts"][f])
        assert (rows[b, :n] >= cases.M).any() and (rows[b, :n] < -1).any() and (T["mp_null"][rows[b, :n][(rows[b, :n] >= 0) & (rows[b, :n] < cases.M)]]).any()
