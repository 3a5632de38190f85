"""Vocabulary training on the device (csrc/voc_train.hip through se2gpu_voc_train / Vocabulary.train) against the host mirror
ORBVocabulary::create (tests/cpp_voc_train.cpp, compiled -O2).  The rule: the exported tree - parents, descriptors, weights,
leaf flags - and the statistics equal the mirror's bit for bit, on every case of tests/voc_train_cases.py; each case first
asserts from the numpy model (tests/voc_train_model.py, which tests/test_voc_train.py holds the mirror to) that its input hits
what it is for.  Nothing here reads the reference's tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bow_gpu as tb  # noqa: E402
import voc_train_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = vc.build_cases()
SOME = ["golden2-root2000", "root2049-k2-L6-idf", "dups-short-seeding-binary"]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("voc_train_gpu")
    exe, r = vc.compile_mirror(d)
    assert r.returncode == 0, r.stderr
    return d, exe, {}


def mirror(work, name):
    """the mirror's result of a case and the file it saved, computed once"""
    d, exe, cache = work
    if name not in cache:
        docs, k, L, wt, sc, seed, max_iters, extra, _ = CASES[name]
        path = d / (name + ".voc")
        cache[name] = (vc.run_mirror(exe, d, docs, k, L, wt, sc, seed, max_iters, voc_out=path), path)
    return cache[name]


def device(name, on_device=False):
    from se2lam_amd import capi
    from se2lam_amd.vocabulary import Vocabulary
    docs, k, L, wt, sc, seed, max_iters, extra, _ = CASES[name]
    desc, counts, cap = vc.pad_docs(docs, extra)
    if not on_device:
        return Vocabulary.train(desc, counts, k, L, wt, sc, seed, max_iters)
    d_desc, d_cnt = capi.DeviceArray.from_numpy(desc), capi.DeviceArray.from_numpy(counts)
    return Vocabulary.train(d_desc.ptr, d_cnt.ptr, k, L, wt, sc, seed, max_iters, cap=cap, nframes=len(counts))


def assert_equal_tree(voc, want):
    parent, desc, weight, leaf = voc.export()
    assert voc.train_stats == want["stats"]
    assert np.array_equal(parent, want["parent"])
    assert np.array_equal(desc[1:], want["desc"][1:])
    assert np.array_equal(leaf, want["leaf"])
    assert np.array_equal(weight, want["weight"])


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_mirror(work, name):
    m = vc.model_of(CASES[name])
    assert CASES[name][8](m), (name, m["stats"], m["ties"])
    want, _ = mirror(work, name)
    assert want["stats"] == m["stats"]
    voc = device(name)
    print(name, voc.train_stats)
    assert (voc.nodes, voc.words, voc.k, voc.L, voc.scoring, voc.weighting) == (want["stats"]["nodes"], want["stats"]["words"]) + CASES[name][1:3] + (CASES[name][4], CASES[name][3])
    assert_equal_tree(voc, want)


@pytest.mark.parametrize("name", SOME)
def test_device_input_equals_host_input(work, name):
    assert_equal_tree(device(name, on_device=True), mirror(work, name)[0])


@pytest.mark.parametrize("name", SOME[:2])
def test_two_runs_are_equal(name):
    a, b = device(name), device(name)
    assert a.train_stats == b.train_stats
    for x, y in zip(a.export(), b.export()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", SOME[:2])
def test_save_load_export_round_trip(work, name):
    from se2lam_amd.vocabulary import Vocabulary
    d = work[0]
    voc = device(name)
    path = d / (name + ".device.voc")
    voc.save(path)
    assert path.read_bytes() == mirror(work, name)[1].read_bytes()      # the file the mirror's saveToBinaryFile wrote
    back = Vocabulary.load(path)
    assert (back.nodes, back.words, back.k, back.L, back.scoring, back.weighting) == (voc.nodes, voc.words, voc.k, voc.L, voc.scoring, voc.weighting)
    for x, y in zip(voc.export(), back.export()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", SOME[:2])
def test_transform_on_the_trained_handle_equals_the_mirror(work, name):
    """the trained vocabulary is a vocabulary: se2gpu_bow_transform on the handle se2gpu_voc_train returned against the mirror's
    transform with the tree it trained"""
    from se2lam_amd.vocabulary import BowContext
    d, _, cache = work
    want, path = mirror(work, name)
    if "bow_exe" not in cache:
        import subprocess
        cache["bow_exe"] = str(d / "cpp_bow_mirror")
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(vc.ROOT, "include"), os.path.join(vc.ROOT, "tests", "cpp_bow_mirror.cpp"), "-o",
                            cache["bow_exe"], "-pthread"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    docs = [x for x in CASES[name][0] if len(x)][:3]
    desc, counts, cap = vc.pad_docs(docs, 0)
    ctx = BowContext(device(name), max_features=cap)
    mine = tb.mirror_transform(cache["bow_exe"], path, desc, counts, 2, d)
    for f, doc in enumerate(docs):
        w, v, (n, p, i) = ctx.transform(doc, 2)
        mw, mv, (mn, mp, mi) = mine[f]
        assert len(w) > 0 and np.array_equal(w, mw) and np.array_equal(v, mv)
        assert np.array_equal(n, mn) and np.array_equal(p, mp) and np.array_equal(i, mi)


def test_device_class_create_equals_host_class(tmp_path):
    """the C++ class: create(vector<vector<Row>>, ...) and saveToBinaryFile on the device and on the host, files equal"""
    import subprocess
    exe = vc.compile_device_class(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "device = host" in r.stdout, r.stdout + r.stderr


def test_refusals():
    from se2lam_amd import capi
    from se2lam_amd.vocabulary import Vocabulary
    docs = vc.noisy_docs(3, [20, 20], 5, 0.05)
    desc, counts, cap = vc.pad_docs(docs, 0)
    assert Vocabulary.train(desc, counts, 4, 2).words > 0
    for bad in (dict(k=1), dict(k=33), dict(L=0), dict(L=11), dict(scoring=6), dict(scoring=-1), dict(weighting=4), dict(weighting=-1)):
        p = dict(dict(k=4, L=2, scoring=0, weighting=0), **bad)
        with pytest.raises(capi.Se2GpuError):
            Vocabulary.train(desc, counts, **p)
    with pytest.raises(capi.Se2GpuError):
        Vocabulary.train(desc, np.zeros(2, np.int32), 4, 2)                      # no descriptor at all
    big = np.zeros((1, 4097, 32), np.uint8)
    with pytest.raises(capi.Se2GpuError):
        Vocabulary.train(big, np.array([4097], np.int32), 4, 2)                  # a document beyond se2gpu_bow's 4096
    assert Vocabulary.train(big, np.array([4096], np.int32), 4, 1, weighting=1).words >= 1   # 4096 copies of one descriptor
    voc = Vocabulary.train(desc, counts, 4, 2)
    n = voc.nodes
    parent, d32, w, leaf = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.zeros(n), np.zeros(n, np.uint8)
    rc = capi.lib().se2gpu_voc_export(voc._h, n - 1, parent.ctypes.data, d32.ctypes.data, w.ctypes.data, leaf.ctypes.data)
    assert rc != 0
