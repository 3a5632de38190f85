"""se2gpu_map_apply_batch_device on the GPU against tests/map_apply_model.py: every output word of every hand-stated case
(tests/map_apply_cases.py: cap 16 to 64, 6 to 8 frames, 48 to 96 point slots, 1 to 4 jobs; one table of 3,000 slots whose scan
spans a dozen workgroups; one point with 70 entries; one table of 66,000 frame slots of one feature), the reference's eleven transitions, run-to-run and batch-position
independence, the padded table under the covisibility and parallax calls, and the new-key-frame chain with a single wait.
Integers are exact and floats equal to the bit: the call copies floats and runs map_normal.h's text, which the model restates
operation by operation."""
import ctypes as C

import numpy as np
import pytest

import map_apply_cases as mc
import map_apply_golden as mg
import map_apply_model as mm

pytestmark = pytest.mark.gpu
S = mm


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


@pytest.fixture(scope="module")
def results(matcher):
    """every case once: (case, model, device)"""
    from se2lam_amd import mapapply
    out = {}
    for name, make in mc.CASES.items():
        c = make()
        out[name] = (c, mm.apply(c), mapapply.apply_case(matcher, c))
    return out


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_equals_the_model_in_every_word(results, name):
    c, want, got = results[name]
    print(name, "sizes_out", got["sizes_out"].tolist())
    mc.compare(got, want, name)


def test_capacity_status_leaves_the_tables_as_they_were(results):
    for name in ("capacity_points", "capacity_entries"):
        c, want, got = results[name]
        assert got["sizes_out"][S.STATUS] == 2
        for k in mm.INPLACE:
            assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.ascontiguousarray(c[k]).view(np.uint8)), (name, k)


def test_an_erase_pass_with_nothing_to_erase_returns_the_table(matcher):
    from se2lam_amd import mapapply
    c = mm.set_jobs(mc.base(), [])
    got = mapapply.apply_case(matcher, c)
    assert got["sizes_out"].tolist() == [0, 4, 7, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(got["mp_ptr_new"][:5], c["mp_ptr"][:5]) and np.array_equal(got["obs_frame_new"][:7], c["obs_frame"][:7])
    mc.compare(got, mm.apply(c), "erase pass")


def test_the_reference_map_in_two_calls_per_transition(matcher):
    """the golden's eleven transitions on one resident table: add, then erase with the pruned key frame null, the second call
    taking its sizes from the first one's d_sizes_out; the states equal the recorded ones and the model's words"""
    from se2lam_amd import capi, mapapply
    g = mg.Golden()
    c = g.first_case()
    dm = mapapply.DeviceMap(c, max_jobs=1)
    for t in g.transitions:
        c = g.add_case(c, t)
        rows = mapapply.upload_rows(c)
        dm.apply(matcher, rows, 14)
        o = mm.apply(c)
        c = g.erase_case(c, o, t)
        dm.frame_null = capi.upload(c["frame_null"], np.uint8)
        dm.apply(matcher, None)
        matcher.sync()
        got, want = dm.download(), mm.apply(c)
        mc.compare(got, want, "transition %d" % t["index"], prefix=True)
        g.check_state(got, t)
        c = mm.next_case(c, want)
    assert t["index"] == 10


def test_the_same_bytes_in_a_second_run(results, matcher):
    from se2lam_amd import mapapply
    for name in ("random_scan", "two_jobs_one_point", "long_list", "capacity_points"):
        c, _, first = results[name]
        again = mapapply.apply_case(matcher, c)
        for k in mm.OUT_FIELDS:
            assert np.array_equal(np.asarray(again[k]).view(np.uint8), np.asarray(first[k]).view(np.uint8)), (name, k)


def test_a_job_alone_and_as_the_third_of_three(matcher):
    """slots shift by the earlier jobs' points and nothing else changes"""
    from se2lam_amd import mapapply

    def rows_of_job(c, b):
        mc.row(c, b, 9, 1, 7)
        mc.row(c, b, 3, 2, 0)
        mc.row(c, b, 4, 3, 12, good=0)
        return mc.row(c, b, 6, 3, 10)
    alone = rows_of_job(mc.base(jobs=((2, 5),)), 0)
    batch = mc.base(jobs=((1, 3), (0, 4), (2, 5)))
    mc.row(batch, 0, 8, 3, 10)
    mc.row(batch, 1, 4, 3, 12)
    mc.row(batch, 1, 2, 3, 13)
    rows_of_job(batch, 2)
    for k in ("view", "info", "new_pos_w", "info_prev", "local_pos", "good_prl_row"):   # the same floats, whatever the job's index
        batch[k][2] = alone[k][0]
    a, b = mapapply.apply_case(matcher, alone), mapapply.apply_case(matcher, batch)
    mc.compare(a, mm.apply(alone), "alone")
    mc.compare(b, mm.apply(batch), "batch")
    shift = 3
    assert a["sizes_out"][S.M_NEW] == 6 and b["sizes_out"][S.M_NEW] == 6 + shift
    assert np.array_equal(a["job_counts"][0], b["job_counts"][2]) and a["job_counts"][0].tolist() == [0, 1, 1, 2, 0, 0]
    la = mm.lists_of(a["mp_ptr_new"], a["obs_frame_new"], a["obs_ftr_new"], 6)
    lb = mm.lists_of(b["mp_ptr_new"], b["obs_frame_new"], b["obs_ftr_new"], 9)
    assert la[:4] == lb[:4] and la[4:] == lb[7:]
    for k in ("pos", "good_prl", "mp_null", "mp_normal", "new_frame"):
        assert np.array_equal(a[k][:4].view(np.uint8), b[k][:4].view(np.uint8)), k
        assert np.array_equal(a[k][4:6].view(np.uint8), b[k][7:9].view(np.uint8)), k
    cap = alone["cap"]
    for f in (2, 5):
        sl = slice(f * cap, (f + 1) * cap)
        fa, fb = a["ftr_mp"][sl], b["ftr_mp"][sl]
        assert np.array_equal(np.where(fa >= 4, fa + shift, fa), fb)
        for k in ("kf_observed", "view_pos", "view_info"):
            assert np.array_equal(a[k][sl].view(np.uint8), b[k][sl].view(np.uint8)), (k, f)
    ea, eb = a["mp_ptr_new"][4], b["mp_ptr_new"][7]
    for k in ("obs_view_new", "obs_info_new"):
        assert np.array_equal(a[k][ea:ea + 4].view(np.uint32), b[k][eb:eb + 4].view(np.uint32)), k


def test_the_padded_table_under_the_covisibility_calls(results, matcher):
    """se2gpu_covis_build_device and se2gpu_covis_pairs_device on the call's output with m = m_cap, nobs = nobs_cap against the
    set model on the exact-size table"""
    import covis_model as cm
    from se2lam_amd import covis
    for name in ("random_small", "two_jobs_one_point", "erase_null_frame_and_add", "long_list"):
        c, _, got = results[name]
        m, n = (int(v) for v in got["sizes_out"][1:3])
        assert m < c["m_cap"] and n < c["nobs_cap"]
        cv = covis.build_device(matcher, c["counts"], c["cap"], got["mp_ptr_new"], got["obs_frame_new"], got["obs_ftr_new"],
                                got["mp_null"], got["good_prl"])
        assert cv.m == c["m_cap"] and cv.nobs == c["nobs_cap"]
        model = cm.Model(c["counts"], c["cap"], got["mp_ptr_new"][:m + 1], got["obs_frame_new"][:n], got["obs_ftr_new"][:n],
                         got["mp_null"][:m], got["good_prl"][:m])
        nf = c["nframes"]
        pa, pb = (np.repeat(np.arange(nf), nf).astype(np.int32), np.tile(np.arange(nf), nf).astype(np.int32))
        d, w = covis.pairs_device(matcher, cv, pa, pb), model.pairs(pa, pb)
        assert np.array_equal(d["out"], w["out"]) and cm.same_floats(d["ratio"], w["ratio"]), name
        assert np.array_equal(cv.read_size_obs(), model.size_obs()) and w["out"][:, 0].max() > 0, name
        W = (m + 63) // 64
        assert np.array_equal(cv.read_bits()[:, :W], model.bits()) and not cv.read_bits()[:, W:].any(), name


# ---- the chain of a new key frame: correspd passes = 1, apply, parallax, apply, correspd passes = 6, apply ----------------

def _chain_case(cc):
    """a map that fits tests/new_kf_cases.py's CorrespdCases: slots 0..Q-1 are its map-point table (one entry each, the main
    observation), then one point per tracked feature; the abandoned point holds (2, 39) and (6, 0)"""
    import new_kf_cases as nc
    Q = len(cc.mp["main_frame"])
    lists = [[(int(f), int(k))] for f, k in zip(cc.mp["main_frame"], cc.mp["main_ftr"])]
    ab = [tuple(e) for e in cc.abandoned["entries"][:2]]
    lists.append(ab)
    for o in np.flatnonzero(cc.observed):
        f, k = divmod(int(o), nc.CAP)
        if (f, k) not in ab:
            lists.append([(f, k)])
    c = mm.blank_case(nc.CAP, len(cc.sc.fr.counts), 176, 448)
    c["counts"][:] = cc.sc.fr.counts
    mm.set_lists(c, lists)
    c["view_pos"][:] = cc.view_pos
    rng = np.random.default_rng(5)
    c["mp_normal"][:len(lists)] = rng.normal(size=(len(lists), 3)).astype(np.float32)
    c["good_prl"][:] = 0
    good_row = rng.integers(0, 2, (len(cc.JOBS), nc.CAP)).astype(np.uint8)
    return c, Q, good_row


def _run_chain(matcher, cc, case, good_row, on_device):
    """the six steps on one set of device tables; on_device: the three applies are the device call and nothing waits before
    the end.  Otherwise every apply waits, downloads, runs the model and uploads what it rebuilt."""
    import new_kf_cases as nc
    import new_kf_model as nk
    from se2lam_amd import capi, mapapply, newkf
    from se2lam_amd.capi import dev_ptr as P, upload as up
    lib, fr, B, cap = capi.lib(), cc.sc.fr, len(cc.JOBS), nc.CAP
    frames = newkf.DevicePoses(fr.kps, fr.counts, fr.cap, fr.Tcw, fr.Twc, fr.P, fr.idkf)
    mi = cc.match_idx_mp.copy()
    mi[0, cc.abandoned["j"]] = cc.abandoned["q"]
    ins = dict(Tcr=up(cc.Tcr, np.float32), Trc=up(cc.Trc, np.float32), matched12=up(cc.matched12, np.int32), mi=up(mi, np.int32),
               inv=up(np.full(B * cap, -9, np.int32)), counts=up(np.full(5 * B, -9, np.int32)))
    table = [up(cc.mp[k], dt) for k, dt in (("main_frame", np.int32), ("main_ftr", np.int32), ("main_octave", np.int32),
                                            ("normal", np.float32), ("dist", np.float32))]
    host_rows = dict(job_prev=cc.job_prev, job_new=cc.job_new, kind=np.full((B, cap), 9, np.uint8), src=np.full((B, cap), -9, np.int32),
                     view=np.full((B, cap, 3), nk.SENT, np.float32), info=np.full((B, cap, 9), nk.SENT, np.float32),
                     new_pos_w=np.full((B, cap, 3), nk.SENT, np.float32), info_prev=np.full((B, cap, 9), nk.SENT, np.float32),
                     local_pos=cc.local_pos, good_prl_row=good_row)
    rows = mapapply.upload_rows(host_rows)
    status = up(np.full(case["m_cap"], -9, np.int32))
    place = up(np.full(case["m_cap"], -9, np.int32))
    st = dict(dm=mapapply.DeviceMap(case, max_jobs=B), cur=case, waits=0, log=[])

    def correspd(passes):
        dm = st["dm"]
        capi.check(lib.se2gpu_kf_correspd_batch_device(
            matcher._h, P(frames.kps_un), P(frames.counts), cap, frames.nframes, P(frames.Tcw), P(frames.Twc), P(frames.P),
            P(dm.feature["kf_observed"]), P(dm.feature["view_pos"]), P(rows["job_prev"]), P(rows["job_new"]), P(ins["Tcr"]),
            P(ins["Trc"]), P(ins["matched12"]), P(rows["local_pos"]), P(ins["mi"]), B, *[P(x) for x in table], len(cc.mp["main_frame"]),
            nc.FX, nc.LOWER, nc.UPPER, passes, P(ins["inv"]), P(rows["kind"]), P(rows["src"]), P(rows["view"]), P(rows["info"]),
            P(rows["new_pos_w"]), P(rows["info_prev"]), P(ins["counts"])))

    def parallax():
        dm = st["dm"]
        capi.check(lib.se2gpu_mappoint_parallax_batch_device(
            matcher._h, P(frames.kps_un), P(frames.counts), cap, frames.nframes, P(frames.Tcw), P(frames.Twc), P(frames.P),
            P(frames.idkf), P(dm.old["mp_ptr"]), P(dm.old["obs_frame"]), P(dm.old["obs_ftr"]), dm.m_cap, dm.nobs_cap,
            P(dm.point["good_prl"]), P(dm.new_frame), nc.FX, nc.LOWER, nc.UPPER, P(dm.feature["kf_observed"]), P(status), P(place),
            P(dm.point["pos"]), P(dm.old["obs_view"]), P(dm.old["obs_info"])))

    def apply(with_rows, kinds, with_status):
        if on_device:
            st["dm"].apply(matcher, rows if with_rows else None, kinds, status if with_status else None)
            return
        matcher.sync()
        st["waits"] += 1
        state = st["dm"].download()
        c = dict(st["cur"])
        for k in mm.INPLACE:
            c[k] = state[k]
        for k in ("mp_ptr", "obs_frame", "obs_ftr", "obs_view", "obs_info"):
            c[k] = state[k + "_new"]
        c["sizes_in"] = state["sizes_out"][1:3].copy()
        c["kinds"] = kinds
        if with_rows:
            mm.set_jobs(c, list(cc.JOBS))
            for k, dt in mapapply.ROW_FIELDS[2:]:
                c[k] = rows[k].to_numpy(dt, host_rows[k].shape)
        else:
            mm.set_jobs(c, [])
        c["has_status"] = with_status
        c["parallax_status"] = status.to_numpy(np.int32, (case["m_cap"],)) if with_status else np.zeros(case["m_cap"], np.int32)
        o = mm.apply(c)
        assert o["sizes_out"][S.STATUS] == 0
        st["log"].append((c, o))
        st["cur"] = mm.next_case(c, o)
        st["dm"] = mapapply.DeviceMap(st["cur"], max_jobs=B)
        st["dm"].new_frame = up(o["new_frame"], np.int32)

    correspd(1)
    apply(True, 2, False)
    parallax()
    apply(False, 14, True)
    correspd(6)
    apply(True, 12, False)
    matcher.sync()
    out = st["dm"].download(B)
    out["parallax_status"] = status.to_numpy(np.int32, (case["m_cap"],))
    out["parallax_place"] = place.to_numpy(np.int32, (case["m_cap"],))
    out["kind"] = rows["kind"].to_numpy(np.uint8, (B, cap))
    out["src"] = rows["src"].to_numpy(np.int32, (B, cap))
    return out, st


def test_the_new_key_frame_chain_with_one_wait(matcher):
    """correspd passes = 1 -> apply (kind 1) -> parallax on the padded table with the call's d_new_frame -> apply (B = 0, the
    statuses) -> correspd passes = 6 -> apply (kinds 2, 3), nothing waited for in between, against the same steps with the table
    rebuilt by the model between them.  The tracked point seen from frames 2 and 6 is abandoned at age 6 by the parallax
    update; its feature of the new key frame is freed and taken by pass 2 for another point."""
    import new_kf_cases as nc
    import new_kf_model as nk
    cc = nc.CorrespdCases(abandoned=True)
    case, Q, good_row = _chain_case(cc)
    dev, _ = _run_chain(matcher, cc, case, good_row, True)
    ref, st = _run_chain(matcher, cc, case, good_row, False)
    assert st["waits"] == 3
    keys = mm.INPLACE + ["mp_ptr_new", "obs_frame_new", "obs_ftr_new", "obs_view_new", "obs_info_new", "new_frame"]
    want = dict(ref)
    want["sizes_out"] = st["log"][-1][1]["sizes_out"]
    assert np.array_equal(dev["sizes_out"][1:3], ref["sizes_out"][1:3])
    mc.compare(dev, want, "chain", keys=keys, prefix=True)
    for k in ("parallax_status", "parallax_place", "kind", "src"):
        assert np.array_equal(dev[k], ref[k]), k
    # the abandoned point: slot Q; null at the end, its features free, feature j of frame 8 with the point pass 2 matched
    ab, cap = cc.abandoned, nc.CAP
    assert dev["parallax_status"][Q] == 2 and (np.delete(dev["parallax_status"], Q) != 2).all()
    assert dev["mp_null"][Q] == 1 and dev["mp_ptr_new"][Q] == dev["mp_ptr_new"][Q + 1]
    assert dev["ftr_mp"][2 * cap + 39] == -1 and dev["ftr_mp"][6 * cap + ab["i"]] == -1 and dev["kf_observed"][2 * cap + 39] == 0
    assert dev["kind"][0, ab["j"]] == 2 and dev["ftr_mp"][8 * cap + ab["j"]] == ab["q"]
    # the parallax call on the padded table equals the model on the exact-size lists with the new observation added
    c1, o1 = st["log"][0]
    m, n = (int(v) for v in o1["sizes_out"][1:3])
    kf_obs = o1["kf_observed"].copy()
    mp = nk.parallax_batch(nk.L64, cc.sc.fr, o1["mp_ptr_new"][:m + 1], o1["obs_frame_new"][:n], o1["obs_ftr_new"][:n],
                           o1["good_prl"][:m], o1["new_frame"][:m], nc.FX, nc.LOWER, nc.UPPER, kf_obs)
    assert np.array_equal(dev["parallax_status"][:m], mp["status"]) and (dev["parallax_status"][m:] == 0).all()
    assert np.array_equal(dev["parallax_place"][:m], mp["place"])
    none = o1["new_frame"][:m] < 0                                        # the call's -1 went to both: no appended entry, nothing done
    assert none.any() and (~none).any() and (dev["parallax_status"][:m][none] == 0).all()
    # and the three steps of the mapping thread changed the map as the jobs' counts say
    c3, o3 = st["log"][2]
    assert o3["sizes_out"][S.CREATED] == o3["job_counts"][:, 3].sum() > 20 and o3["job_counts"][0, 2] >= 3
    assert np.array_equal(dev["job_counts"], o3["job_counts"])
