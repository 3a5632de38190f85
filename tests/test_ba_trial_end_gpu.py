"""The end of a Levenberg-Marquardt trial on the multi-launch paths of csrc/ba.hip, per pose model and launch shape: the
force-stop flag, a run of zero iterations and the synchronous controller (a notification per trial) for the SE(2) model (the
finisher workgroup of k_update), the SE3-expmap model (k6_finalize<Expmap>), the pose graph (k6_finalize<PoseGraph>) and a sharded SE(2) run
(k_finalize + k_lm_decide).  One contract - g2o's solve loop - for all of them."""
import numpy as np
import pytest

import pg_cases
from ba_cases import LM_REJECT_CASES, REJECT, env, kidnapped, kidnapped3, opt, opt3, pg, sharded_equals_single

pytestmark = pytest.mark.gpu

# model -> (handle of a graph, the smallest graph the generator makes for it, a start whose trials get rejected)
MODELS = {
    "se2": (opt, lambda s: s.ba_graph(8, 60), lambda s: kidnapped(s, *LM_REJECT_CASES[2][0])),
    "se3": (opt3, lambda s: s.ba3_graph(8, 60, 0), lambda s: kidnapped3(s, *REJECT)),
    "pose_graph": (pg, lambda s: s.pose_graph(12), lambda s: pg_cases.rejecting(24, 1, 7)),
}


def _same_to_the_bit(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("model", list(MODELS))
def test_stop_flag_and_zero_iterations(synth, model):
    """setForceStopFlag (LocalMapper.cpp:246) raised before the run: no iteration, `stopped`, the cost of the start, the
    estimates untouched; lowered again the same handle runs like a fresh one, to the bit.  optimize(0) evaluates the start."""
    make, graph, _ = MODELS[model]
    g = graph(synth)
    with env(SE2GPU_BA_RESIDENT="0"):   # (the SE3 model: the multi-launch path, as ba_cases.multi_launch takes it)
        o = make(g)
        start = o.estimates()
        flag = np.ones(1, np.uint8)
        o.setForceStopFlag(flag)
        assert o.optimize(10) == 0
        assert o.stats["stopped"]
        assert o.stats["chi2_final"] == o.stats["chi2_init"]
        assert _same_to_the_bit(o.estimates(), start)
        fresh = make(g)
        fresh.optimize(4)
        flag[0] = 0
        o.optimize(4)
        assert not o.stats["stopped"]
        assert o.stats == fresh.stats, (o.stats, fresh.stats)
        assert _same_to_the_bit(o.estimates(), fresh.estimates())
        z = make(g)
        assert z.optimize(0) == 0
        assert z.stats["chi2_init"] == fresh.stats["chi2_init"]


@pytest.mark.parametrize("model", list(MODELS))
def test_synchronous_controller_equals_the_asynchronous_one(synth, model):
    """setVerbose(True) = the synchronous controller: the host reads the controller block after EVERY trial (each slot ends with
    a notification) and enqueues only what the next trial needs.  On a start that rejects trials it takes the decisions of the
    asynchronous run."""
    make, graph, reject = MODELS[model]
    g = (reject or graph)(synth)
    with env(SE2GPU_BA_RESIDENT="0"):
        a = make(g)
        a.optimize(10)
        v = make(g)
        v.setVerbose(True)
        v.optimize(10)
    sa, sv = a.stats, v.stats
    if reject is not None:
        assert max(sa["trials_hist"]) > 1, sa["trials_hist"]   # the fixture: trials were rejected
    assert sv["trials_hist"] == sa["trials_hist"]
    assert sv["iterations"] == sa["iterations"] and sv["terminated"] == sa["terminated"]
    # two paths of one model are held to 1e-9 relative elsewhere (RTOL of test_ba_window_se3_gpu); these two run the same kernels
    # on the same sums in the same order, and the histories have been equal to the bit since the tests were written
    assert sv["chi2_hist"] == sa["chi2_hist"]
    assert sv["lambda_hist"] == sa["lambda_hist"]


def test_sharded_stop(synth):
    """Two landmark shards on one GPU with the flag raised on both ranks before the run: k_lm_decide's stop branch.  No
    iteration on either rank, `stopped`, the replicated poses untouched."""
    g = synth.ba_graph(8, 60)
    single, results = sharded_equals_single(g, 10, stop=np.ones(1, np.uint8))
    assert single.stats["iterations"] == 0 and single.stats["stopped"]
    for st, (poses, _) in results:
        assert st["iterations"] == 0 and st["stopped"]
        assert np.array_equal(poses, g.poses)
