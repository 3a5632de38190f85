"""se2gpu_local_ba_batch_device on the GPU: the gather against the numpy statement of Map::loadLocalGraph
(tests/local_graph_model.py) on every case of tests/local_ba_cases.py, read through se2gpu_local_ba_ws_layout; the results against
the host route (lists and tables on the host -> se2gpu_local_graph -> se2gpu_ba_load_local_graph -> initialize ->
se2gpu_ba_optimize_batch) on the resident and on the multi-launch path, at the tolerances tests/test_ba_window_gpu.py holds the
resident kernel to; the chain build -> connect -> window -> local BA on one stream with one wait; and the existing batch paths
before and after a device-route call, bit for bit.

Integers, poses, e_uv and o_meas are exact (float -> double conversions); e_info and o_info are held to 1e-10 relative, the figure
the project holds loadLocalGraph's information to (the model rounds every operation, the kernel is built without contraction)."""
import numpy as np
import pytest

import local_ba_cases as lc
import local_graph_model as lg
from ba_cases import env

pytestmark = pytest.mark.gpu
INFO_RTOL = 1e-10
EXACT = ("fixed", "poses", "o_i", "o_j", "o_meas", "lm_ptr", "e_kf", "e_uv", "lms")
ITERS = 10


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


def _device(matcher, T, jobs, caps, iters=ITERS, mode=0, dT=None, sync=True):
    from se2lam_amd import localba as lb
    rows = lc.job_rows(jobs, caps["kf_list_cap"], caps["mp_list_cap"])
    return lb.local_ba_device(matcher, dT or lb.device_tables(T), rows[0], rows[1], rows[2], rows[3], caps["kf_list_cap"], rows[4],
                              caps["mp_list_cap"], K=T["K"], Tbc12=T["Tbc12"], huber=T["huber"], xrot_info=T["xrot_info"],
                              z_info=T["z_info"], iters=iters, mode=mode, max_local=caps["max_local"], max_ref=caps["max_ref"],
                              max_mp=caps["max_mp"], max_obs=caps["max_obs"], sync=sync)


def _model(T, jobs, caps):
    rows = lc.job_rows(jobs, caps["kf_list_cap"], caps["mp_list_cap"])
    return lg.batch(T, *rows, caps)


def _same_gather(got, j, want, what):
    """job j of a device result against the model's graph"""
    from se2lam_amd import capi
    status = int(got["status"][j])
    assert status == want["status"], (what, status, want["status"])
    assert got["info"][j].tolist() == want["counts"].tolist(), (what, got["info"][j], want["counts"])
    g = got["gather"](j)
    assert g["counts"].tolist() == want["counts"].tolist(), what
    if status in (0, 5):
        for k in EXACT:
            assert g[k].dtype == want[k].dtype and np.array_equal(g[k], want[k]), (what, k)
        for k in ("e_info", "o_info"):
            assert g[k].shape == want[k].shape and np.allclose(g[k], want[k], rtol=INFO_RTOL, atol=0), (what, k)
    if status == 5:                                              # the outputs are the start values
        P, L = int(want["counts"][0]), int(want["counts"][2])
        assert np.array_equal(got["kf_out"][j, :P], want["poses"]) and np.array_equal(got["mp_out"][j, :L], want["lms"]), what
        assert (got["kf_out"][j, P:] == capi.SENT).all() and (got["mp_out"][j, L:] == capi.SENT).all(), what
    if status in (1, 2, 3, 4):                                   # not run: the outputs are left alone
        assert (got["kf_out"][j] == capi.SENT).all() and (got["mp_out"][j] == capi.SENT).all(), what
    if status != 0:
        assert got["stats"][j]["iterations"] == 0 and got["stats"][j]["chi2_init"] == 0.0, what


def _groups(case):
    """the jobs of a case by the caps they are run with: [(caps, [job index])]"""
    groups = {}
    for j in range(len(case["jobs"])):
        over = case["job_caps"][j] if "job_caps" in case else {}
        groups.setdefault(tuple(sorted(over.items())), []).append(j)
    return [(dict(case["caps"], **dict(k)), js) for k, js in groups.items()]


@pytest.mark.parametrize("name", sorted(lc.cases()))
def test_gather_equals_the_model(matcher, name):
    case = lc.cases()[name]
    statuses = []
    for caps, js in _groups(case):
        jobs = [case["jobs"][j] for j in js]
        got, want = _device(matcher, case["T"], jobs, caps), _model(case["T"], jobs, caps)
        for i, j in enumerate(js):
            _same_gather(got, i, want[i], (name, j))
            assert want[i]["status"] == case["expect"][j]["status"], (name, j)
            statuses.append(int(got["status"][i]))
    assert len(statuses) == len(case["jobs"])


def test_a_landmark_of_more_than_64_edges_is_refused_by_the_gather_and_its_neighbour_runs(matcher):
    case = lc.wide_landmark_case()
    got, want = _device(matcher, case["T"], case["jobs"], case["caps"]), _model(case["T"], case["jobs"], case["caps"])
    assert [w["status"] for w in want] == [4, 0] and want[0]["counts"][3] > 64
    for j in range(2):
        _same_gather(got, j, want[j], ("wide", j))
    alone = _device(matcher, case["T"], case["jobs"][1:], case["caps"])
    _same_results(got, 1, alone, 0, "the job next to a refused one")
    assert got["stats"][1]["iterations"] == ITERS and np.isfinite(got["kf_out"][1, :int(want[1]["counts"][0])]).all()


def _bytes_of(g):
    return {k: v.tobytes() for k, v in g.items()}


def _same_results(a, i, b, j, what):
    """two runs of the resident kernel on the same graph: its sums are LDS atomics, so equal to rounding (the tolerances of
    tests/test_ba_window_gpu.py), with the same decisions"""
    sa, sb = a["stats"][i], b["stats"][j]
    assert sa["trials_hist"] == sb["trials_hist"] and sa["iterations"] == sb["iterations"], what
    assert np.allclose(sa["chi2_hist"], sb["chi2_hist"], rtol=1e-9) and np.isclose(sa["chi2_init"], sb["chi2_init"], rtol=1e-9), what
    assert np.allclose(a["kf_out"][i], b["kf_out"][j], rtol=1e-9, atol=1e-7) and np.allclose(a["mp_out"][i], b["mp_out"][j], rtol=1e-9, atol=1e-6), what


def test_a_jobs_words_do_not_depend_on_its_place_or_on_the_run(matcher):
    c = lc.cases()
    T = c["ref_present"]["T"]
    job, other, third = c["ref_present"]["jobs"][0], c["caps"]["jobs"][0], c["all_fixed"]["jobs"][0]
    caps = lc.CAPS
    alone = _device(matcher, T, [job], caps)
    first = _device(matcher, T, [job, other, third], caps)
    last = _device(matcher, T, [third, other, job], caps)
    again = _device(matcher, T, [third, other, job], caps)
    assert alone["status"].tolist() == [0] and first["status"].tolist() == [0, 0, 5] and last["status"].tolist() == [5, 0, 0]
    ref = _bytes_of(alone["gather"](0))
    for got, j, what in ((first, 0, "job 0 of 3"), (last, 2, "job 2 of 3"), (again, 2, "a second run")):
        assert _bytes_of(got["gather"](j)) == ref, what
        assert got["info"][j].tolist() == alone["info"][0].tolist(), what
    # (the solver's sums are LDS atomics: its results agree to rounding, which the next test holds; the gather has no atomics)


# ---- the host route ------------------------------------------------------------------------------------------------------------

def _host_route(T, job, iters, resident):
    from se2lam_amd import localba as lb, optimizer as op
    with env(SE2GPU_BA_RESIDENT="1" if resident else "0"):
        o = op.SlamOptimizer()
        op.loadLocalGraph(o, **lb.flatten_local_graph(T, job["local"], job["ref"], job["mps"]))
        o.initializeOptimization(0)
        op.optimize_batch([o], iters)
        from se2lam_amd import capi
        assert (capi.lib().se2gpu_ba_last_batch_path() == 2) == resident
        return o.stats, o.estimates()


def _same_as_host(got, j, st, est, what):
    d = got["stats"][j]
    n = st["iterations"]
    assert d["iterations"] == n and d["trials"] == st["trials"] and d["trials_hist"] == st["trials_hist"], (what, d["trials_hist"], st["trials_hist"])
    assert d["terminated"] == st["terminated"] and d["stopped"] == st["stopped"], what
    assert np.isclose(d["chi2_init"], st["chi2_init"], rtol=1e-9), (what, d["chi2_init"], st["chi2_init"])
    assert np.allclose(d["chi2_hist"][:n], st["chi2_hist"][:n], rtol=1e-9), (what, d["chi2_hist"], st["chi2_hist"])
    assert np.allclose(d["lambda_hist"][:n], st["lambda_hist"][:n], rtol=1e-7), what
    P, L = est[0].shape[0], est[1].shape[0]
    assert np.allclose(got["kf_out"][j, :P], est[0], rtol=1e-9, atol=1e-7), what
    assert np.allclose(got["mp_out"][j, :L], est[1], rtol=1e-9, atol=1e-6), what


def _result_windows():
    """(T, job, rejects): windows with and without reference key frames and odometry, and a start Levenberg-Marquardt rejects
    trials on (a local key frame moved by metres and tens of degrees, as ba_cases.kidnapped does)"""
    c = lc.cases()
    base = c["ref_present"]["T"]
    kid = lc.kidnap(base, **lc.KIDNAP)
    return [(base, c["ref_present"]["jobs"][0], False), (c["no_ref_least_id_and_id_1"]["T"], c["no_ref_least_id_and_id_1"]["jobs"][0], False),
            (c["frame_twice"]["T"], c["frame_twice"]["jobs"][0], False), (base, c["caps"]["jobs"][0], False),
            (kid, lc.window(kid, 3, [2, 3, 4]), True)]


@pytest.mark.parametrize("resident", [True, False])
def test_results_equal_the_host_route(matcher, resident):
    for k, (T, job, rejects) in enumerate(_result_windows()):
        got = _device(matcher, T, [job], lc.CAPS)
        assert got["status"].tolist() == [0], k
        st, est = _host_route(T, job, ITERS, resident)
        assert (max(st["trials_hist"]) > 1) == rejects, (k, st["trials_hist"])
        _same_as_host(got, 0, st, est, (k, resident))
        assert len(est[0]) == got["info"][0, 0] and len(est[1]) == got["info"][0, 2]


def test_gauss_newton_and_a_batch_of_three(matcher):
    wins = _result_windows()
    T = wins[0][0]
    jobs = [wins[0][1], wins[3][1], wins[0][1]]
    got = _device(matcher, T, jobs, lc.CAPS, iters=4, mode=1)
    assert got["status"].tolist() == [0, 0, 0]
    from se2lam_amd import optimizer as op, localba as lb
    for j, job in enumerate(jobs):
        with env(SE2GPU_BA_RESIDENT="1"):
            o = op.SlamOptimizer()
            op.loadLocalGraph(o, **lb.flatten_local_graph(T, job["local"], job["ref"], job["mps"]))
            o.initializeOptimization(0)
            op.optimize_batch([o], 4, mode=1)
        _same_as_host(got, j, o.stats, o.estimates(), ("gn", j))


# ---- the chain -----------------------------------------------------------------------------------------------------------------

def test_chain_on_the_stream_with_one_wait(matcher):
    """se2gpu_covis_build_device -> se2gpu_covis_connect_device -> se2gpu_local_window_batch_device -> se2gpu_local_ba_batch_device
    queued on the matcher's stream with a single se2gpu_matcher_sync at the end: the local-BA call reads the lists where the
    window call left them in device memory"""
    from se2lam_amd import covis, localba as lb, localwindow as lw
    T = lc.cases()["ref_present"]["T"]
    nframes, m = len(T["counts"]), len(T["pos"])
    caps = dict(lc.CAPS, max_ref=nframes, kf_list_cap=nframes, mp_list_cap=m)
    pa, pb = np.array([2, 3], np.int32), np.array([3, 4], np.int32)       # 2 - 3 - 4 covisible: one hop from 3 gives [2, 3, 4]
    jobs = np.array([3, 6], np.int32)
    order = np.argsort(T["frame_id"], kind="stable").astype(np.int32)
    cv = covis.DeviceCovis(T["counts"], T["cap"], T["mp_ptr"], T["obs_frame"], T["obs_ftr"]).build(matcher, sync=False)
    adj = lw.DeviceAdjacency(nframes).connect(matcher, pa, pb, None, 1, sync=False)
    win = lw.window_device(matcher, cv, adj, jobs, 1, frame_null=T["frame_null"], kf_order=order, kf_list_cap=nframes, mp_list_cap=m,
                           sync=False)
    d_jobs, d_out, d_ll, d_rl, d_ml = (win.arrays[k] for k in ("job_kf", "out", "local_list", "ref_list", "mp_list"))
    dT = lb.device_tables(T)
    p = lb.local_ba_device(matcher, dT, d_jobs, d_out, d_ll, d_rl, nframes, d_ml, m, K=T["K"], Tbc12=T["Tbc12"], huber=T["huber"],
                           iters=ITERS, max_local=caps["max_local"], max_ref=caps["max_ref"], max_mp=caps["max_mp"],
                           max_obs=caps["max_obs"], sync=False)
    matcher.sync()
    w, got = win.read(), p.read()
    assert w["out"][0, :3].tolist() == [3, 4, 16] and w["local_list"][0, :3].tolist() == [2, 3, 4]
    assert got["status"].tolist() == [0, 0]
    for j, cur in enumerate(jobs):
        job = dict(cur=int(cur), local=w["local_list"][j, :w["out"][j, 0]].tolist(), ref=w["ref_list"][j, :w["out"][j, 1]].tolist(),
                   mps=w["mp_list"][j, :w["out"][j, 2]].tolist())
        assert got["info"][j, 3] == w["out"][j, 3]              # the edges the window call counted are the edges gathered
        _same_gather(got, j, _model(T, [job], caps)[0], ("chain", j))
        st, est = _host_route(T, job, ITERS, True)
        _same_as_host(got, j, st, est, ("chain", j))


# ---- the existing paths ----------------------------------------------------------------------------------------------------------

def test_the_existing_batch_paths_are_unchanged_by_a_device_route_call(matcher, synth):
    from se2lam_amd import capi, optimizer as op
    from ba_cases import opt
    T, job = _result_windows()[0][:2]
    # path 1 (lock step) takes a batch of two or more SE(2) windows; a batch of one window goes to its own stream, path 0 (the
    # switch that keeps larger batches off the lock-step path is read once per process)
    for path in (0, 1):
        with env(SE2GPU_BA_RESIDENT="0"):
            def run():
                os_ = [opt(synth.ba_graph(8, 60)), opt(synth.ba_graph(12, 200))]
                paths = set()
                for batch in ([os_] if path == 1 else [os_[:1], os_[1:]]):
                    op.optimize_batch(batch, 5)
                    paths.add(int(capi.lib().se2gpu_ba_last_batch_path()))
                return paths, [(o.stats, [a.tobytes() for a in o.estimates()]) for o in os_]
            before = run()
            assert before[0] == {path}
            got = _device(matcher, T, [job], lc.CAPS)
            assert got["status"].tolist() == [0]
            after = run()
            assert before == after, path


# ---- a camera off the body's axes ----------------------------------------------------------------------------------------------

def _off_axis_window():
    """the map and window of the case ref_present (the same random draws), seen through synth.OFF_AXIS_TBC / OFF_CENTRE_CAM: Rcw
    in the gathered informations and Rcb in the solver are full matrices, the principal point is off the image centre"""
    from se2lam_amd import synth
    f, cx, cy = synth.OFF_CENTRE_CAM
    T = lc.scene(2, 10, 36, Tbc12=np.r_[synth.OFF_AXIS_TBC[:3, :3].reshape(-1), synth.OFF_AXIS_TBC[:3, 3]],
                 K=np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32))
    return T, lc.window(T, 3, [2, 3, 4])


def test_off_axis_camera_gather_equals_the_model_and_results_equal_the_host_route(matcher):
    T, job = _off_axis_window()
    assert np.abs(T["Tbc12"][:9]).min() > 0.02 and np.abs(T["Tcw"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).min() > 0.02
    used = [(f, k) for p in job["mps"] for f, k in zip(lc.observers(T, p), T["obs_ftr"][T["mp_ptr"][p]:T["mp_ptr"][p + 1]])]
    assert min(T["view_pos"][f, k, 2] for f, k in used) >= 300.0
    got, want = _device(matcher, T, [job], lc.CAPS), _model(T, [job], lc.CAPS)
    assert want[0]["status"] == 0
    _same_gather(got, 0, want[0], "off axis")
    for resident in (True, False):
        st, est = _host_route(T, job, ITERS, resident)
        _same_as_host(got, 0, st, est, ("off axis", resident))
