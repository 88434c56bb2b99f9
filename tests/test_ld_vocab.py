"""The vocabulary side of the loop detector without a GPU: csrc/ld_vocab.h under the address and undefined-behaviour sanitizers
(tests/native/ld_vocab_check.cpp, a stand-alone program), the Python holder's file layout, the exported symbols and the structures."""
import ctypes as C
import os
import subprocess

import numpy as np

import vplines_slam_amd as v

import ld_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VPL_E_INVALID = -1
NAMES = ["vpl_ld_default_options", "vpl_ld_create", "vpl_ld_destroy", "vpl_ld_set_vocabulary", "vpl_ld_load_vocabulary", "vpl_ld_detect",
         "vpl_ld_detect_fe", "vpl_ld_add", "vpl_ld_reset", "vpl_ld_size", "vpl_ld_get_bow"]


def test_ld_vocab_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ld_vocab_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "vplines-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "ld_vocab_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ld vocab ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_vocabulary_file_layout_and_round_trip(tmp_path):
    voc = ld_inputs.regular_vocabulary(3, 2, seed=1, weighting=v.frontend.IDF, shuffle=True)
    path = str(tmp_path / "voc.bin")
    voc.to_file(path)
    raw = open(path, "rb").read()
    n, w = len(voc.node_id), len(voc.word_id)
    assert (n, w) == (12, 9) and len(raw) == 24 + 48 * n + 8 * w
    assert np.frombuffer(raw, "<i4", 6).tolist() == [3, 2, 0, v.frontend.IDF, n, w]
    # the second node record, field by field
    assert np.frombuffer(raw, "<i4", 2, 24 + 48).tolist() == [int(voc.node_id[1]), int(voc.parent_id[1])]
    assert np.frombuffer(raw, "<f8", 1, 24 + 48 + 8)[0] == voc.weight[1]
    assert np.array_equal(np.frombuffer(raw, "<u8", 4, 24 + 48 + 16), voc.descriptor[1])
    assert np.frombuffer(raw, "<i4", 2, 24 + 48 * n + 8 * 2).tolist() == [int(voc.word_node[2]), int(voc.word_id[2])]
    back = v.Vocabulary.from_file(path)
    assert (back.k, back.L, back.scoring, back.weighting) == (3, 2, 0, v.frontend.IDF)
    for name in ("node_id", "parent_id", "weight", "descriptor", "word_node", "word_id"):
        assert np.array_equal(getattr(back, name), getattr(voc, name)), name
    open(path, "wb").write(raw[:-1])
    try:
        v.Vocabulary.from_file(path)
        assert False, "a truncated file was read"
    except ValueError as e:
        assert "truncated" in str(e)


def test_symbols_structures_and_null_arguments():
    lib = v.load_hip_library()
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert v.LoopDetector is v.frontend.LoopDetector
    # 5 ints (20, padded to 24) | 2 doubles;  6 ints | 4 doubles | 2 ints
    assert C.sizeof(v.LoopDetectorOptions) == 40 and v.LoopDetectorOptions.neighbour_score.offset == 24
    assert C.sizeof(v.LoopDetectorResult) == 64 and v.LoopDetectorResult.scores.offset == 24 and v.LoopDetectorResult.n_words.offset == 56
    o = v.default_loop_detector_options()
    assert (o.max_results, o.recent, o.neighbour_score, o.loop_score) == (4, 50, 0.05, 0.015)
    assert o.max_keypoints == 8192 and o.max_keyframes >= 1 and o.max_words_total >= 1
    h = C.c_void_p()
    assert lib.vpl_ld_create(C.byref(h), None, 1, C.byref(o)) == VPL_E_INVALID and not h.value
    assert lib.vpl_ld_detect(None, None, None, None, None) == VPL_E_INVALID
    assert lib.vpl_ld_detect_fe(None, None, None) == VPL_E_INVALID
    assert lib.vpl_ld_add(None, None, None, None) == VPL_E_INVALID
    assert lib.vpl_ld_set_vocabulary(None, 0, 0, 0, 0, 0, None, None, None, None, 0, None, None) == VPL_E_INVALID
    assert lib.vpl_ld_load_vocabulary(None, None) == VPL_E_INVALID
    assert lib.vpl_ld_reset(None, 0) == VPL_E_INVALID and lib.vpl_ld_size(None, 0) == VPL_E_INVALID
    assert lib.vpl_ld_get_bow(None, 0, 0, None, None, None) == VPL_E_INVALID
    lib.vpl_ld_destroy(None)   # a no-op
