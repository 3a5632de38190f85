"""tests/local_graph_model.py, the numpy statement of Map::loadLocalGraph the device gather is held to, against expectations
stated by hand on every case of tests/local_ba_cases.py, against the compiled restatement of Map.cpp:1024-1049
(oracle.ba_edge_information, which test_ref_compiled.py holds to the compiled reference at 1e-10), and against the graphs the
compiled reference's own Map::loadLocalGraph built (tests/golden/local_graph_ref.npz, written by tools/gen_local_graph_golden.py)."""
import os

import numpy as np
import pytest

import local_ba_cases as lc
import local_graph_model as lg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_graph_ref.npz")


def _run(case):
    caps = case["caps"]
    rows = lc.job_rows(case["jobs"], caps["kf_list_cap"], caps["mp_list_cap"])
    out = []
    for j in range(len(case["jobs"])):
        c = dict(caps, **(case["job_caps"][j] if "job_caps" in case else {}))
        r = lc.job_rows(case["jobs"][j:j + 1], c["kf_list_cap"], c["mp_list_cap"])
        out.append(lg.load_local_graph(case["T"], int(r[0][0]), r[1][0], r[2][0], r[3][0], r[4][0], c))
    assert len(rows[0]) == len(out)
    return out


@pytest.mark.parametrize("name", sorted(lc.cases()))
def test_cases_against_hand_stated_expectations(name):
    case = lc.cases()[name]
    got = _run(case)
    assert [g["status"] for g in got] == [e["status"] for e in case["expect"]], name
    for g, e, job in zip(got, case["expect"], case["jobs"]):
        if g["status"] in (1, 2, 3, 4):
            assert g["fixed"] is None and g["e_kf"] is None
            continue
        nl, nr, L = len(job["local"]), len(job["ref"]), len(job["mps"])
        assert g["counts"][0] == nl + nr and g["counts"][2] == L and g["counts"][7] == 0
        # vertex numbering: local key frame i -> i, reference key frame i -> n_local + i; reference key frames are fixed
        assert g["fixed"][nl:].all() and len(g["fixed"]) == nl + nr
        assert np.array_equal(g["poses"], case["T"]["Twb"][job["local"] + job["ref"]].astype(np.float64))
        assert np.array_equal(g["lms"], case["T"]["pos"][job["mps"]].astype(np.float64))
        assert g["lm_ptr"][0] == 0 and g["lm_ptr"][-1] == len(g["e_kf"]) == g["counts"][3] and (np.diff(g["lm_ptr"]) >= 0).all()
        assert ((g["e_kf"] >= 0) & (g["e_kf"] < nl + nr)).all()
        for l in range(L):                                      # a key frame observes a point once
            kfs = g["e_kf"][g["lm_ptr"][l]:g["lm_ptr"][l + 1]].tolist()
            assert len(set(kfs)) == len(kfs)
        if "local" in e:
            assert job["local"] == e["local"]
        if "fixed" in e:
            assert g["fixed"][:nl].tolist() == e["fixed"]
        if "n_fixed_local" in e:
            assert int(g["fixed"][:nl].sum()) == e["n_fixed_local"]
        if "odo" in e:
            assert list(zip(g["o_i"].tolist(), g["o_j"].tolist())) == e["odo"]
        if "empty_point" in e:
            assert g["lm_ptr"][e["empty_point"] + 1] == g["lm_ptr"][e["empty_point"]]
        for l, d in e.get("degree", {}).items():
            assert g["lm_ptr"][l + 1] - g["lm_ptr"][l] == d
        if "skipped_at_least" in e:
            assert g["counts"][5] >= e["skipped_at_least"]
        assert g["counts"][6] == e.get("flags", 0)
        if "not_ref" in e:
            assert e["not_ref"] not in job["ref"]
        if g["status"] == 5:
            assert g["counts"][1] == 0 or g["counts"][3] + g["counts"][4] == 0


def test_every_rule_has_a_case():
    c = lc.cases()
    got = {n: _run(c[n]) for n in c}
    statuses = {g["status"] for r in got.values() for g in r}
    assert statuses == {0, 1, 2, 3, 5}
    w = lc.wide_landmark_case()
    r = _run(w)
    assert [g["status"] for g in r] == [4, 0]
    assert r[0]["counts"][3] > 64 and r[0]["counts"][0] == 2 + len(w["jobs"][0]["ref"]) >= 2 + 66
    assert r[0]["lm_ptr"] is None and r[1]["lm_ptr"] is not None and np.diff(r[1]["lm_ptr"]).max() <= 64
    # odometry information: the closed-form inverse is an inverse
    g = got["odometry_null_target"][0]
    T = c["odometry_null_target"]["T"]
    for i, info in zip(g["o_i"], g["o_info"]):
        slot = c["odometry_null_target"]["jobs"][0]["local"][i]
        assert np.allclose(info @ T["odo_cov"][slot].reshape(3, 3), np.eye(3), rtol=0, atol=1e-9)
    # an entry that the octave rule skips keeps its frame taken: the edges of the point are those of its other observers
    g = got["octave_out_of_range"][0]
    assert g["counts"][6] == 1 and g["counts"][5] >= 2


def test_information_equals_the_compiled_restatement(oracle):
    """Map.cpp:1024-1049 as oracle/ compiled it from the reference's expressions (Eigen), on the edges of two windows"""
    for name in ("ref_present", "no_ref_least_id_and_id_1"):
        case = lc.cases()[name]
        T, job = case["T"], case["jobs"][0]
        g = _run(case)[0]
        slots = job["local"] + job["ref"]
        # the edges again, as flat inputs of the restatement
        lcs, lws, s2 = [], [], []
        at = 0
        for l, p in enumerate(job["mps"]):
            seen = set()
            for f, k in lg.point_entries(T, p):
                if f in slots and f not in seen and lg.entry_valid(T, f, k):
                    seen.add(f)
                    assert g["e_kf"][at] == slots.index(f)
                    lcs.append(T["view_pos"][f, k]); lws.append(T["pos"][p]); s2.append(T["level_sigma2"][T["kps_octave"][f, k]])
                    at += 1
        assert at == len(g["e_kf"]) > 20
        Rcw = T["Tcw"][slots].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9)
        want = oracle.ba_edge_information(lc=np.array(lcs), lw=np.array(lws), e_kf=g["e_kf"], sigma2=np.array(s2), Rcw=Rcw,
                                          twb_xy=T["Twb"][slots][:, :2], fx=float(T["K"][0, 0]), xrot_info=T["xrot_info"], z_info=T["z_info"])
        got = np.stack([g["e_info"][:, 0], g["e_info"][:, 1], g["e_info"][:, 1], g["e_info"][:, 2]], axis=1).reshape(-1, 2, 2)
        assert np.allclose(got, want, rtol=1e-10, atol=0), name


def golden_maps(path=GOLDEN):
    """[(T, job, ref)]: the tables, the window's lists and the compiled reference's graph of every recorded map"""
    z = np.load(path)
    maps = []
    for i in range(int(z["nmaps"][0])):
        g = lambda k: z["m%d_%s" % (i, k)]  # noqa: E731
        cfg = g("cfg")
        T = {k: g(k) for k in ("frame_id", "Twb", "Tcw", "odo_to", "odo_meas", "odo_cov", "kps_xy", "kps_octave", "counts", "view_pos",
                               "level_sigma2", "pos", "mp_ptr", "obs_frame", "obs_ftr", "K", "Tbc12")}
        T.update(frame_null=None, cap=T["kps_octave"].shape[1], huber=float(cfg[0]), xrot_info=float(cfg[1]), z_info=float(cfg[2]))
        job = dict(cur=int(cfg[3]), local=g("local").tolist(), ref=g("ref").tolist(), mps=g("mps").tolist())
        maps.append((T, job, {k: g(k) for k in ("v_est", "v_fixed", "o_ids", "o_meas", "o_info", "e_ids", "e_uv", "e_info")}))
    return maps


def test_model_equals_the_compiled_reference():
    """Map::loadLocalGraph of the compiled reference on maps built with its own calls (tests/golden/local_graph_ref.npz): the vertex
    numbering, the fixed rule, the poses and points, the PreSE2 edges with cov^-1, and per EdgeSE2XYZ the key frame, the measurement
    and the information.  Integers and converted floats exact, informations to 1e-10 relative.  The reference walks a point's
    observers in std::set<PtrKeyFrame> order - the order of the heap - so its edges are matched by (key frame, point)."""
    maps = golden_maps()
    assert 20 <= len(maps) <= 50
    caps = dict(max_local=12, max_ref=12, max_mp=64, max_obs=400, kf_list_cap=12, mp_list_cap=64)
    seen_fixed_local = seen_no_ref = 0
    for i, (T, job, ref) in enumerate(maps):
        rows = lc.job_rows([job], caps["kf_list_cap"], caps["mp_list_cap"])
        g = lg.load_local_graph(T, int(rows[0][0]), rows[1][0], rows[2][0], rows[3][0], rows[4][0], caps)
        P, L = len(job["local"]) + len(job["ref"]), len(job["mps"])
        assert g["status"] in (0, 5), i
        assert np.array_equal(g["fixed"], ref["v_fixed"][:P]) and not ref["v_fixed"][P:].any(), i
        assert np.array_equal(g["poses"], ref["v_est"][:P]) and np.array_equal(g["lms"], ref["v_est"][P:]), i
        assert np.array_equal(np.stack([g["o_i"], g["o_j"]], axis=1), ref["o_ids"].reshape(-1, 2)), i
        assert np.array_equal(g["o_meas"], ref["o_meas"]), i
        assert np.allclose(g["o_info"], ref["o_info"], rtol=1e-10, atol=0), i
        e_lm = np.repeat(np.arange(L), np.diff(g["lm_ptr"]))
        mine = {(int(k), int(l)): e for e, (k, l) in enumerate(zip(g["e_kf"], e_lm))}
        assert len(mine) == len(g["e_kf"]) == len(ref["e_ids"]) and set(mine) == set(map(tuple, ref["e_ids"].tolist())), i
        for ids, uv, W in zip(ref["e_ids"].tolist(), ref["e_uv"], ref["e_info"]):
            e = mine[tuple(ids)]
            assert np.array_equal(g["e_uv"][e], uv), (i, ids)
            assert np.allclose([g["e_info"][e, 0], g["e_info"][e, 1], g["e_info"][e, 1], g["e_info"][e, 2]], W.reshape(-1), rtol=1e-10, atol=0), (i, ids)
        seen_fixed_local += bool(job["ref"] and g["fixed"][:len(job["local"])].any())
        seen_no_ref += not job["ref"]
    assert seen_fixed_local >= 1 and seen_no_ref >= 3
