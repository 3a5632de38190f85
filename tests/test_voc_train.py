"""Vocabulary training on the host (include/se2lam_amd/VocabularyTrain.h, ORBVocabulary::create).

1. The rules are the reference's: tests/voc_train_model.py with alias=True (the reference's shallow-copy defect, emulated) and
   the recorded rand() stream equals the vocabulary file that the reference's compiled DBoW2 wrote, on the three cases of
   tests/golden/voc_train_dbow2.npz (tools/gen_voc_train_golden.py) - parents, descriptors, leaf flags, float weights, with ==.
2. The host mirror equals the model with value semantics and counter draws, bit for bit, stats included, on the cases of
   tests/voc_train_cases.py; each case first asserts from the model that it hits what it is for.
3. The same driver built with -fsanitize=address,undefined as a stand-alone program runs two cases clean.
4. The refusals of VocabularyTrain.h.
5. A mirror-trained file loads in the reference's compiled DBoW2 (oracle/ref.py), whose transform of the training documents
   equals the mirror's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voc_train_cases as vc  # noqa: E402
import voc_train_model as vm  # noqa: E402

CASES = vc.build_cases()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("voc_train")
    exe, r = vc.compile_mirror(d)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.fixture(scope="module")
def models():
    return {}


def model(models, name):
    if name not in models:
        models[name] = vc.model_of(CASES[name])
    return models[name]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_model_with_the_reference_defect_equals_the_compiled_dbow2(i):
    docs, k, L, wt, sc, seed, rand, blob = vc.golden_case(i)
    gk, gL, gsc, gwt, parent, desc, weight, leaf = vc.parse_voc(blob)
    assert (gk, gL, gsc, gwt) == (k, L, sc, wt)
    rng = vm.Stream(rand)
    m = vm.train(docs, k, L, wt, rng, alias=True)
    assert rng.at == len(rand)                       # every recorded draw was consumed, none was missing
    assert len(m["parent"]) == len(parent)
    assert np.array_equal(m["parent"][1:], parent[1:])
    assert np.array_equal(m["desc"][1:], desc[1:])
    assert np.array_equal(m["leaf"][1:], leaf[1:])
    assert m["weight"].dtype == np.float32 and np.array_equal(m["weight"][1:], weight[1:])


@pytest.mark.parametrize("name", list(CASES))
def test_mirror_equals_model(work, models, name):
    d, exe = work
    docs, k, L, wt, sc, seed, max_iters, extra, expect = CASES[name]
    m = model(models, name)
    assert expect(m), (name, m["stats"], m["ties"])
    got = vc.run_mirror(exe, d, docs, k, L, wt, sc, seed, max_iters)
    assert got is not None
    assert got["stats"] == m["stats"]
    assert np.array_equal(got["parent"], m["parent"])
    assert np.array_equal(got["desc"][1:], m["desc"][1:])
    assert np.array_equal(got["leaf"], m["leaf"])
    assert np.array_equal(got["weight"], m["weight"].astype(np.float64))


def test_all_weightings_and_the_listed_k_and_L_are_covered():
    ks, Ls, wts = {c[1] for c in CASES.values()}, {c[2] for c in CASES.values()}, {c[3] for c in CASES.values()}
    assert {2, 10, 32} <= ks and {1, 3, 6} <= Ls and wts == {0, 1, 2, 3}


def test_mirror_under_sanitizers(tmp_path, models):
    exe, r = vc.compile_mirror(tmp_path, flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), name="cpp_voc_train_san")
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitizer" in r.stderr.lower()):
        pytest.skip("the sanitizer runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for name in ("golden1-empty", "dups-short-seeding-binary"):
        docs, k, L, wt, sc, seed, max_iters, extra, _ = CASES[name]
        got = vc.run_mirror(exe, tmp_path, docs, k, L, wt, sc, seed, max_iters)   # a sanitizer report ends the program with an error
        assert got["stats"] == model(models, name)["stats"]


def test_refusals(work):
    d, exe = work
    docs = vc.noisy_docs(3, [20, 20], 5, 0.05)
    ok = dict(k=4, L=2, wt=0, sc=0)
    assert vc.run_mirror(exe, d, docs, ok["k"], ok["L"], ok["wt"], ok["sc"], 1) is not None
    for bad in (dict(k=1), dict(k=33), dict(L=0), dict(L=11), dict(sc=6), dict(sc=-1), dict(wt=4), dict(wt=-1)):
        p = dict(ok, **bad)
        assert vc.run_mirror(exe, d, docs, p["k"], p["L"], p["wt"], p["sc"], 1) is None, bad
    empty = [np.zeros((0, 32), np.uint8)] * 3
    assert vc.run_mirror(exe, d, empty, 4, 2, 0, 0, 1) is None
    big = [np.random.default_rng(0).integers(0, 256, (4097, 32), dtype=np.uint8)]
    assert vc.run_mirror(exe, d, big, 4, 2, 0, 0, 1) is None
    big[0] = big[0][:4096]
    assert vc.run_mirror(exe, d, big, 4, 1, 1, 0, 1) is not None


def test_device_class_create_compiles_and_links(tmp_path):
    """ORBVocabularyDevice::create / saveToBinaryFile over the C ABI; without a device the program reports the refusal"""
    exe = vc.compile_device_class(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_trained_file_loads_in_the_compiled_dbow2(work):
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref is not built and the reference's tree is not here to build it from")
    d, exe = work
    docs, k, L, wt, sc, seed, max_iters, extra, _ = CASES["golden1-empty"]
    path = d / "trained.bin"
    got = vc.run_mirror(exe, d, docs, k, L, wt, sc, seed, max_iters, voc_out=path)
    rv = ref.RefVocabulary(path)
    assert rv.loaded and (rv.k, rv.L, rv.scoring, rv.weighting) == (k, L, sc, wt)
    assert rv.words in (got["stats"]["words"], got["stats"]["words"] + 1)   # its loader appends one phantom record (ORBVocabulary.h, deviations)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_bow_gpu as tb
    bexe = str(d / "cpp_bow_mirror")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(vc.ROOT, "include"), os.path.join(vc.ROOT, "tests", "cpp_bow_mirror.cpp"), "-o", bexe,
                        "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    desc, counts, cap = vc.pad_docs(docs, 0)
    mine = tb.mirror_transform(bexe, path, desc, counts, 1, d)
    for f, doc in enumerate(docs):
        w, v, fv = rv.transform(doc, 1)
        mw, mv, (mn, mp, mi) = mine[f]
        assert w == mw.tolist() and np.array_equal(v, mv)
        assert fv == {int(mn[i]): mi[mp[i]:mp[i + 1]].tolist() for i in range(len(mn))}
