"""CPU tests of the device vocabulary's boundary (se2gpu.h, section "DBoW2 vocabulary"): the header declares the functions and
the library exports them, they fail loudly without a device, the C++ class over them (include/se2lam_amd/ORBVocabularyDevice.h)
compiles and links as plain C++17, and the host vocabulary still refuses and accepts what it did - its file checks now live in
include/se2lam_amd/VocabularyTree.h, shared with se2gpu_voc_load / se2gpu_voc_create."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["se2gpu_voc_create", "se2gpu_voc_load", "se2gpu_voc_destroy", "se2gpu_voc_words", "se2gpu_voc_nodes", "se2gpu_voc_k", "se2gpu_voc_L",
       "se2gpu_voc_scoring", "se2gpu_voc_weighting", "se2gpu_bow_create", "se2gpu_bow_destroy", "se2gpu_bow_set_stream", "se2gpu_bow_sync",
       "se2gpu_bow_stream", "se2gpu_bow_transform_batch_device", "se2gpu_bow_transform", "se2gpu_bowdb_create", "se2gpu_bowdb_destroy",
       "se2gpu_bowdb_add", "se2gpu_bowdb_add_device", "se2gpu_bowdb_remove", "se2gpu_bowdb_size", "se2gpu_bowdb_query"]


def test_header_declares_and_library_exports_the_vocabulary_calls():
    from se2lam_amd import capi
    txt = open(os.path.join(ROOT, "include", "se2gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(se2gpu_[A-Za-z0-9_]+)\s*\(", txt))
    lib = capi.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name


def test_no_device_no_vocabulary(tmp_path):
    from se2lam_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    from se2lam_amd import vocabulary as V
    parent, desc, weight, leaf = V.synthetic_vocabulary(0, 3, 2)
    with pytest.raises(capi.Se2GpuError) as e:
        V.Vocabulary(3, 2, 0, 0, parent, desc, weight, leaf)
    assert e.value.code == capi.ERR_NO_DEVICE
    path = tmp_path / "voc.bin"
    V.write_vocabulary_file(path, 3, 2, 0, 0, parent, desc, weight, leaf)
    with pytest.raises(capi.Se2GpuError) as e:
        V.Vocabulary.load(path)
    assert e.value.code == capi.ERR_NO_DEVICE
    h = C.c_void_p()
    lib = capi.lib()
    assert lib.se2gpu_bow_create(None, 100, 1, C.byref(h)) == capi.ERR_NO_DEVICE and not h
    assert lib.se2gpu_bowdb_create(None, C.byref(h)) == capi.ERR_NO_DEVICE and not h
    assert lib.se2gpu_voc_create(3, 2, 0, 0, len(parent), None, None, None, None, None) == capi.ERR_INVALID
    assert lib.se2gpu_voc_words(None) == capi.ERR_INVALID and lib.se2gpu_bowdb_size(None) == capi.ERR_INVALID


def test_device_vocabulary_class_compiles_and_links(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_bow_device")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_bow_device_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def _mirror(tmp_path):
    exe = str(tmp_path / "cpp_bow_mirror")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_bow_mirror.cpp"), "-o", exe, "-pthread"])
    return exe


def test_shared_file_checks_refuse_what_the_host_vocabulary_refused(tmp_path):
    """the four refusals of ORBVocabulary::loadFromBinaryFile, through the header both sides now share, and a childless node
    that is not a leaf; a well-formed file with early leaves and short sibling lists loads"""
    from se2lam_amd import vocabulary as V
    exe = _mirror(tmp_path)
    parent, desc, weight, leaf = V.synthetic_vocabulary(9, 4, 3, full=False, early_leaf=0.2)
    good = tmp_path / "voc.bin"
    V.write_vocabulary_file(good, 4, 3, 0, 0, parent, desc, weight, leaf)
    blob = good.read_bytes()
    frames = struct.pack("<iii", 1, 4, 4) + desc[1:5].tobytes()
    (tmp_path / "in.bin").write_bytes(frames)
    last_leaf = 24 + 41 * (len(parent) - 2) + 40
    assert blob[last_leaf] == 1
    cases = {"truncated": blob[:-17], "node size": blob[:4] + struct.pack("<I", 40) + blob[8:],
             "forward parent": blob[:24] + struct.pack("<i", 5) + blob[28:], "empty": b"",
             "scoring out of range": blob[:16] + struct.pack("<i", 6) + blob[20:],
             "childless inner node": blob[:last_leaf] + b"\x00" + blob[last_leaf + 1:]}
    for name, data in cases.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        r = subprocess.run([exe, "transform", str(p), str(tmp_path / "in.bin"), "1", str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "LOAD failed" in r.stdout, name
    r = subprocess.run([exe, "transform", str(good), str(tmp_path / "in.bin"), "1", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = (tmp_path / "o.bin").read_bytes()
    nb = struct.unpack_from("<i", out)[0]
    assert 1 <= nb <= 4


def test_synthetic_vocabulary_is_what_it_says():
    from se2lam_amd import vocabulary as V
    parent, desc, weight, leaf = V.synthetic_vocabulary(3, 10, 4)
    assert len(parent) == 11111 and leaf.sum() == 10000 and (np.diff(parent[1:]) >= 0).all() and (parent[1:] < np.arange(1, len(parent))).all()
    assert (np.bincount(parent[1:], minlength=len(parent))[~leaf] == 10).all()
    parent, desc, weight, leaf = V.synthetic_vocabulary(3, 6, 5, full=False, early_leaf=0.15, tie_frac=0.3)
    nch = np.bincount(parent[1:], minlength=len(parent))
    depth = np.zeros(len(parent), int)
    for i in range(1, len(parent)):
        depth[i] = depth[parent[i]] + 1
    assert (nch[~leaf] >= 2).all() and (nch[~leaf] < 6).any() and (nch[leaf] == 0).all()
    assert (depth[leaf] < 5).any() and depth.max() == 5                         # leaves above depth L
    first = np.nonzero(np.diff(parent[1:], prepend=-1))[0] + 1                  # every parent's first child
    assert sum(np.array_equal(desc[c], desc[c + 1]) for c in first if parent[c + 1] == parent[c]) > 10     # tied siblings
    assert ((weight == 0) & leaf).any() and (weight[~leaf] == 0).all()
