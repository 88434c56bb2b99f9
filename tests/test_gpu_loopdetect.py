"""The loop detector session (vpl_ld_*) on the device against tests/ld_ref.py, bit for bit: words, bag values, ids, scores (as
uint64 views) and loop_index."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vplines_slam_amd as v
from vplines_slam_amd.frontend import Vocabulary, TF_IDF, TF, IDF, BINARY

import lc_inputs
import ld_inputs
import ld_ref

pytestmark = pytest.mark.gpu

VPL_E_INVALID, VPL_E_CAPACITY = -1, -4
GUARDS = os.environ.get("VPL_DEBUG_GUARDS") == "1"


class Rig:
    def __init__(self, n_db=1, voc=None, width=64, height=48, max_images=None, **opt):
        opt.setdefault("max_keypoints", 64)
        opt.setdefault("max_keyframes", 128)
        opt.setdefault("max_words_total", 128 * 64)
        self.fe = v.frontend.FrontendContext(max_images=max_images or n_db, width=width, height=height, max_lines=64)
        self.ld = v.LoopDetector(self.fe, n_db, **opt)
        if voc is not None:
            self.ld.set_vocabulary(voc)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if GUARDS and a[0] is None:
            assert self.fe.debug_guards() == 0, "a kernel wrote behind a device array"
        self.fe.close()


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def check_result(got, want, what=""):
    assert got["loop_index"] == want["loop_index"], (what, got, want)
    assert got["ids"].tolist() == list(want["ids"]), (what, got, want)
    assert np.array_equal(bits(got["scores"]), bits(want["scores"])), (what, got, want)
    assert got["n_words"] == want["n_words"] and got["entry"] == want["entry"], (what, got, want)


def check_bag(ld, db, entry, want, what=""):
    words, values = ld.bow(db, entry)
    assert words.tolist() == list(want[0]), (what, entry)
    assert np.array_equal(bits(values), bits(want[1])), (what, entry)


def words_of(x):
    return np.array([ld_inputs.to_words(d) for d in x], np.uint64).reshape(-1, 4)


# ---- the descent alone, through the bags of single-descriptor frames ----
def test_descent_on_irregular_trees():
    parents, descs, probes, notes = ld_inputs.irregular_tree()
    rng = np.random.default_rng(11)
    n = len(parents)
    for order in (None, [int(i) for i in rng.permutation(n)]):      # node ids in file order, and shuffled
        voc = ld_inputs.tree_vocabulary(parents, descs, order=order)
        tree = ld_ref.Tree(voc)
        node_of_word = {int(w): int(nd) for nd, w in zip(voc.word_node, voc.word_id)}
        if order is None:   # the inputs are what they claim to be, on the reference first
            got = {k: node_of_word[tree.descend(ld_inputs.to_words(p))[0]] for k, p in probes.items()}
            assert got["depth1"] == notes["a"] and got["chain"] == notes["chain_leaf"]
            assert got["wide_last"] == notes["wide"][16] and got["wide_first"] == notes["wide"][0]      # child 17: the second pass of 16 lanes
            assert got["twins"] == notes["twins"][0] and got["equidistant"] == notes["eq"][0]            # the first wins
            assert max(np.bincount(parents)) == 17 and 1 in np.bincount(parents)[1:]
        frames = [ld_inputs.to_words(p) for p in probes.values()]
        frames += [ld_inputs.to_words(ld_inputs.rand_desc(rng)) for _ in range(30)]
        frames += [ld_inputs.to_words(ld_inputs.flip(descs[int(rng.integers(n))], 5, rng)) for _ in range(30)]
        with Rig(voc=voc) as r:
            for i, d in enumerate(frames):
                res, = r.ld.add([[d]])
                word, weight = tree.descend(d)
                assert res["n_words"] == 1 and res["entry"] == i
                words, values = r.ld.bow(0, i)
                assert words.tolist() == [word] and values.tolist() == [1.0], (i, word, words)


def test_the_empty_vocabulary_gives_empty_bags():
    voc = Vocabulary(10, 6, [], [], [], np.zeros((0, 4), np.uint64), [], [])
    det = ld_ref.Detector(voc)
    rng = np.random.default_rng(2)
    with Rig(voc=voc) as r:
        for i in range(3):
            f = words_of([ld_inputs.rand_desc(rng) for _ in range(5)])
            res, = r.ld.detect([f], [49])
            check_result(res, det.detect(f, 49))
            assert res["n_words"] == 0 and res["entry"] == i and len(res["ids"]) == 0
            check_bag(r.ld, 0, i, ([], []))


# ---- the bag ----
def near_leaves(voc, words, rng, flips=3):
    leaves = ld_inputs.leaf_descriptors(voc)
    return words_of([ld_inputs.flip(leaves[int(w)], flips, rng) for w in words])


def test_bag_counts_one_word_and_stop_words():
    voc = ld_inputs.sequence_vocabulary()
    at = {int(n): i for i, n in enumerate(voc.node_id)}
    weight = {int(w): float(voc.weight[at[int(n)]]) for n, w in zip(voc.word_node, voc.word_id)}
    stops = [w for w, x in weight.items() if x == 0.0]
    live = [w for w, x in weight.items() if x > 0.0]
    assert len(stops) >= 3
    rng = np.random.default_rng(4)
    MK = 96                                  # no power of two
    frames = [near_leaves(voc, [live[5]] * 40, rng),                 # all on one word
              near_leaves(voc, stops[:3] * 4, rng),                  # stop words only: an empty bag that still takes an entry id
              near_leaves(voc, [live[7], stops[0], live[7], live[2]], rng)]
    for n in (0, 1, 63, 64, 65, MK):
        frames.append(near_leaves(voc, rng.choice(live[:200], n), rng))          # drawn with repetition
    det = ld_ref.Detector(voc)
    with Rig(voc=voc, max_keypoints=MK, max_words_total=1024) as r:
        for i, f in enumerate(frames):
            want = det.detect(f, 49)
            res, = r.ld.detect([f], [49])
            check_result(res, want, i)
            check_bag(r.ld, 0, i, det.entries[i], i)
    assert det.entries[0][0] == [live[5]] and det.entries[0][1] == [1.0]
    assert det.entries[1] == ([], []) and det.entries[2][0] == sorted([live[7], live[2]])
    assert [len(f) for f in frames[3:]] == [0, 1, 63, 64, 65, MK] and len(det.entries[8][0]) < MK


def test_bag_at_the_largest_row():
    """max_keypoints 8192: the bag kernel's LDS is above the default limit of a launch there; a full row and a partly filled one"""
    voc = ld_inputs.sequence_vocabulary()
    leaves = ld_inputs.leaf_descriptors(voc)
    rng = np.random.default_rng(6)
    MK = 8192
    frames = []
    for n, n_words in ((MK, 3000), (5000, 10000)):
        d = np.array([ld_inputs.to_words(leaves[int(w)]) for w in rng.choice(n_words, n)], np.uint64)
        d[np.arange(n), rng.integers(0, 4, n)] ^= np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)       # one bit turned
        frames.append(d)
    det = ld_ref.Detector(voc)
    with Rig(voc=voc, max_keypoints=MK, max_keyframes=4, max_words_total=4 * MK) as r:
        for i, f in enumerate(frames):
            want = det.detect(f, 49)
            res, = r.ld.detect([f], [49])
            check_result(res, want, i)
            check_bag(r.ld, 0, i, det.entries[i], i)
    assert 2000 < len(det.entries[0][0]) < 3000 and len(det.entries[1][0]) > 3000


def added(w, n):
    s = w
    for _ in range(n - 1):
        s += w
    return s


def test_repeated_addition_is_not_the_product():
    """A weight added 3, 5, 7, 11 and 13 times.  From 7 on a weight is searched on the CPU for which the repeated addition differs
    from count * w and the difference survives the normalisation.  For 3 and 5 no such weight exists: w + w and 4 w are exact, 3 w
    is rounded once, and its error is too small to move 3 w + w off 4 w (a tie goes to 4 w, whose mantissa is even then), so the
    fifth term is again one rounding of 5 w; the search asserts that on 10000 weights, and both counts are checked against the
    reference like the others."""
    rng = np.random.default_rng(9)
    picked = {}
    for n in (3, 5, 7, 11, 13):
        for _ in range(10000):
            w = float(rng.uniform(0.01, 10.0))
            s, p = added(w, n), n * w
            if n in (3, 5):
                assert s == p
                picked[n] = w
            elif s != p and s / (s + 1.0) != p / (p + 1.0):
                picked[n] = w
                break
    assert sorted(picked) == [3, 5, 7, 11, 13]
    # root -> node 1 (all zeros, weight w), node 2 (all ones, weight 1)
    ones = (1 << 256) - 1
    for n, w in picked.items():
        voc = ld_inputs.tree_vocabulary([0, 0], [0, ones], weights=[w, 1.0])
        f = words_of([0] * n + [ones])
        want = ld_ref.Tree(voc).transform(f)
        assert want[0] == [0, 1] and want[1][0] == added(w, n) / (added(w, n) + 1.0)
        if n > 5:
            assert want[1][0] != (n * w) / (n * w + 1.0)
        with Rig(voc=voc) as r:
            r.ld.add([f])
            check_bag(r.ld, 0, 0, want, n)


@pytest.mark.parametrize("weighting", [TF_IDF, TF, IDF, BINARY])
def test_each_weighting(weighting):
    voc = ld_inputs.regular_vocabulary(4, 3, seed=21, weighting=weighting, stop_fraction=0.1)
    rng = np.random.default_rng(weighting)
    det = ld_ref.Detector(voc)
    with Rig(voc=voc) as r:
        for i in range(4):
            f = near_leaves(voc, rng.choice(64, 40), rng)            # 40 descriptors on 64 words: repetitions
            want = det.detect(f, 49)
            res, = r.ld.detect([f], [49])
            check_result(res, want, i)
            check_bag(r.ld, 0, i, det.entries[i], i)
    assert any(len(e[0]) < 40 for e in det.entries)


# ---- the 85-keyframe sequence ----
def test_the_sequence_every_result_and_every_bag():
    voc, frames = ld_inputs.sequence_vocabulary(), ld_inputs.sequence()
    want, entries = ld_inputs.sequence_reference()
    named = {48: {47}, 49: set(range(49)), 50: {49}, 51: {0, 50}}      # newest only | all | newest only | < 1 and the newest
    probe = ld_ref.Detector(voc)
    with Rig(voc=voc, max_keypoints=32) as r:
        for i, f in enumerate(frames):
            res, = r.ld.detect([f], [i])
            check_result(res, want[i], i)
            if i in named:
                probe.entries = entries[:i]
                assert set(probe.eligible(i)) == named[i]
                assert set(res["ids"].tolist()) <= named[i], (i, res)
        for i in range(len(frames)):
            check_bag(r.ld, 0, i, entries[i], i)
        assert r.ld.size(0) == 85


def test_ties_go_by_ascending_entry_id():
    voc = ld_inputs.sequence_vocabulary()
    rng = np.random.default_rng(8)
    f = near_leaves(voc, rng.choice(10000, 20, replace=False), rng)
    other = near_leaves(voc, rng.choice(10000, 20, replace=False), rng)
    for max_results, want_ids in ((2, [0, 1]), (4, [0, 1, 3, 4])):          # the cut falls inside the tie
        det = ld_ref.Detector(voc, max_results=max_results)
        with Rig(voc=voc, max_results=max_results) as r:
            for k, g in enumerate([f, f, other, f, f]):
                r.ld.add([g]); det.add(g)
            res, = r.ld.detect([f], [49])
            want = det.detect(f, 49)
            check_result(res, want)
            assert res["ids"].tolist() == want_ids and len(set(bits(res["scores"]).tolist())) == 1


# ---- the batch ----
def batch_run():
    voc = ld_inputs.sequence_vocabulary()
    seqs = [ld_inputs.sequence(), ld_inputs.sequence(shift=2), ld_inputs.sequence(shift=1)]
    out = []
    with Rig(n_db=3, voc=voc, max_keypoints=32) as r:
        for i in range(85):
            briefs = [seqs[0][i], seqs[1][i] if i % 2 == 0 else None, seqs[2][i]]        # database 1 is skipped on odd calls
            out.append(r.ld.detect(briefs, [i, i, i]))
        bags = [[r.ld.bow(d, e) for e in range(r.ld.size(d))] for d in range(3)]
        # reset of one database leaves the others alone
        r.ld.reset(1)
        assert [r.ld.size(d) for d in range(3)] == [85, 0, 85]
        after = r.ld.detect([seqs[0][5], seqs[1][0], None], [85, 85, 85])
        bag0 = r.ld.bow(0, 40)
    return out, bags, after, bag0


def test_batch_independence_reset_and_repeatability():
    voc = ld_inputs.sequence_vocabulary()
    out, bags, after, bag0 = batch_run()
    want0, ent0 = ld_inputs.sequence_reference()
    want2, ent2 = ld_inputs.sequence_reference(shift=1)
    det1 = ld_ref.Detector(voc)
    seq1 = ld_inputs.sequence(shift=2)
    for i in range(85):
        check_result(out[i][0], want0[i], ("db0", i))
        check_result(out[i][2], want2[i], ("db2", i))
        if i % 2 == 0:
            check_result(out[i][1], det1.detect(seq1[i], i), ("db1", i))
        else:
            assert out[i][1]["entry"] == -1 and out[i][1]["loop_index"] == -1 and len(out[i][1]["ids"]) == 0
    assert [len(b) for b in bags] == [85, 43, 85]
    for d, ent in ((0, ent0), (1, det1.entries), (2, ent2)):
        for e, (w, val) in enumerate(bags[d]):
            assert w.tolist() == ent[e][0] and np.array_equal(bits(val), bits(ent[e][1])), (d, e)
    # after the reset: database 0 goes on where it was, database 1 starts again, database 2 is untouched
    d0 = ld_ref.Detector(voc); d0.entries = list(ent0)
    check_result(after[0], d0.detect(ld_inputs.sequence()[5], 85), "db0 after the reset")
    check_result(after[1], ld_ref.Detector(voc).detect(seq1[0], 85), "db1 after the reset")
    assert after[1]["entry"] == 0 and after[2]["entry"] == -1
    assert bag0[0].tolist() == ent0[40][0] and np.array_equal(bits(bag0[1]), bits(ent0[40][1]))
    # two runs give the same bits
    out2, bags2, after2, _ = batch_run()
    for a, b in zip(out + [after], out2 + [after2]):
        for x, y in zip(a, b):
            assert x["loop_index"] == y["loop_index"] and x["ids"].tolist() == y["ids"].tolist()
            assert np.array_equal(bits(x["scores"]), bits(y["scores"])) and x["n_words"] == y["n_words"]
    for d in range(3):
        for (w, val), (w2, val2) in zip(bags[d], bags2[d]):
            assert np.array_equal(w, w2) and np.array_equal(bits(val), bits(val2))


def test_batch_under_debug_guards_in_a_fresh_process():
    """the batch run once more with VPL_DEBUG_GUARDS=1 (read when a context is made): the session's arrays go through the guarded
    allocator, and the pattern behind every one of them is intact when the context is closed"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VPL_DEBUG_GUARDS="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    code = "import test_gpu_loopdetect as t; assert t.GUARDS; t.batch_run(); print('guards ok')"
    r = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "guards ok" in r.stdout


# ---- detect_fe ----
def test_detect_fe_takes_the_rows_the_keyframe_call_left_on_the_device():
    images = lc_inputs.image_cases()["batch3_constant_in_the_middle"]
    voc = ld_inputs.sequence_vocabulary()
    cam = v.frontend.PointCamera(*lc_inputs.CAM)
    none = [np.zeros((0, 2))] * 3
    MK = 1024

    def context():
        r = Rig(n_db=3, voc=voc, width=160, height=120, max_keypoints=MK, max_keyframes=8, max_words_total=8 * MK)
        r.fe.lc_reserve(MK, 16)
        r.fe.lc_set_pattern(*lc_inputs.pattern())
        return r

    with context() as r:
        with pytest.raises(RuntimeError, match="no descriptor rows"):
            r.ld.detect_fe([49, 49, 49])
        kf = r.fe.lc_keyframe(images, none, cam, lc_inputs.FAST_TH)
        first = r.ld.detect_fe([49, 49, 49])
        r.fe.lc_keyframe(images[::-1].copy(), none, cam, lc_inputs.FAST_TH)       # slots 0 and 2 swapped
        second = r.ld.detect_fe([49, 49, 49])
        bags = [[r.ld.bow(d, e) for e in range(2)] for d in range(3)]
    rows = [k["brief"] for k in kf]
    assert len(rows[0]) > 64 and len(rows[1]) == 0 and len(rows[2]) > 64
    with context() as r:
        a = r.ld.detect(rows, [49, 49, 49])
        b = r.ld.detect(rows[::-1], [49, 49, 49])
        for d in range(3):
            check_result(first[d], a[d], d)
            check_result(second[d], b[d], d)
            for e in range(2):
                check_bag(r.ld, d, e, (bags[d][e][0].tolist(), bags[d][e][1]), (d, e))
    for d in range(3):
        det = ld_ref.Detector(voc)
        check_result(first[d], det.detect(rows[d], 49), d)
        check_result(second[d], det.detect(rows[2 - d], 49), d)
    assert first[1]["n_words"] == 0 and first[0]["n_words"] > 32 and len(second[0]["ids"]) == 1
    # shapes that do not fit are refused
    with Rig(n_db=2, voc=voc, width=160, height=120, max_images=3, max_keypoints=MK, max_keyframes=8, max_words_total=8 * MK) as r:
        r.fe.lc_reserve(MK, 16)
        r.fe.lc_set_pattern(*lc_inputs.pattern())
        r.fe.lc_keyframe(images, none, cam, lc_inputs.FAST_TH)
        with pytest.raises(RuntimeError, match=r"\(-1\).*3 images.*2 databases"):
            r.ld.detect_fe([49, 49])
        assert r.ld.size(0) == 0
    with Rig(n_db=3, voc=voc, width=160, height=120, max_keypoints=MK // 2, max_keyframes=8, max_words_total=8 * MK) as r:
        r.fe.lc_reserve(MK, 16)
        r.fe.lc_set_pattern(*lc_inputs.pattern())
        r.fe.lc_keyframe(images, none, cam, lc_inputs.FAST_TH)
        with pytest.raises(RuntimeError, match=r"\(-1\).*rows of 1024"):
            r.ld.detect_fe([49, 49, 49])


# ---- capacity and errors ----
def test_capacity_and_errors_leave_the_databases_as_they_were():
    voc = ld_inputs.sequence_vocabulary()
    frames = ld_inputs.sequence()
    want, entries = ld_inputs.sequence_reference()
    # a call before a vocabulary is set
    with Rig(n_db=1, max_keypoints=32) as r:
        with pytest.raises(RuntimeError, match=r"\(-1\).*no vocabulary"):
            r.ld.detect([frames[0]], [0])
        with pytest.raises(RuntimeError, match=r"\(-1\).*no vocabulary"):
            r.ld.add([frames[0]])
        r.ld.set_vocabulary(voc)
        check_result(r.ld.detect([frames[0]], [0])[0], want[0])
    # keyframe max_keyframes + 1, in database 1 of two: neither database changes
    with Rig(n_db=2, voc=voc, max_keypoints=32, max_keyframes=3, max_words_total=1024) as r:
        for i in range(3):
            r.ld.detect([None, frames[i]], [i, i])
        with pytest.raises(RuntimeError, match=r"\(-4\).*database 1 holds 3 keyframes"):
            r.ld.detect([frames[0], frames[3]], [3, 3])
        assert [r.ld.size(d) for d in range(2)] == [0, 3]
        res = r.ld.detect([frames[0], None], [0, 0])
        check_result(res[0], want[0])
        for i in range(3):
            check_bag(r.ld, 1, i, entries[i])
    # counts above max_keypoints
    with Rig(n_db=1, voc=voc, max_keypoints=31) as r:
        with pytest.raises(RuntimeError, match=r"\(-4\).*database 0: 32 descriptors"):
            r.ld.detect([frames[0]], [0])
        assert r.ld.size(0) == 0
        check_result(r.ld.detect([frames[0][:31]], [0])[0], ld_ref.Detector(voc).detect(frames[0][:31], 0))
    # a pool one word too small for the third bag; with one more word it fits
    need = sum(len(e[0]) for e in entries[:3])
    for pool in (need - 1, need):
        with Rig(n_db=1, voc=voc, max_keypoints=32, max_words_total=pool) as r:
            for i in range(2):
                check_result(r.ld.detect([frames[i]], [i])[0], want[i])
            if pool < need:
                with pytest.raises(RuntimeError, match=r"\(-4\).*database 0: a bag of %d words" % len(entries[2][0])):
                    r.ld.detect([frames[2]], [2])
                assert r.ld.size(0) == 2
                for i in range(2):
                    check_bag(r.ld, 0, i, entries[i])
                # the database is as it was: the same query once more, against a reference that holds two entries
                det = ld_ref.Detector(voc); det.entries = list(entries[:2])
                small = frames[2][:4]
                check_result(r.ld.detect([small], [2])[0], det.detect(small, 2))
            else:
                check_result(r.ld.detect([frames[2]], [2])[0], want[2])
                check_bag(r.ld, 0, 2, entries[2])


def test_a_refused_vocabulary_changes_nothing_and_a_new_one_clears_the_databases(tmp_path):
    voc = ld_inputs.sequence_vocabulary()
    frames = ld_inputs.sequence()
    want, entries = ld_inputs.sequence_reference()
    with Rig(n_db=1, voc=voc, max_keypoints=32) as r:
        for i in range(3):
            r.ld.detect([frames[i]], [i])
        bad = Vocabulary(2, 1, [1, 2], [0, 0], [1.0, 1.0], np.zeros((2, 4), np.uint64), [1, 2], [0, 0])      # word 0 twice
        with pytest.raises(RuntimeError, match=r"\(-1\).*given twice"):
            r.ld.set_vocabulary(bad)
        l2 = Vocabulary(2, 1, [1, 2], [0, 0], [1.0, 1.0], np.zeros((2, 4), np.uint64), [1, 2], [0, 1], scoring=1)
        with pytest.raises(RuntimeError, match=r"\(-1\).*L1_NORM"):
            r.ld.set_vocabulary(l2)
        path = str(tmp_path / "voc.bin")
        voc.to_file(path)
        cut = str(tmp_path / "cut.bin")
        open(cut, "wb").write(open(path, "rb").read()[:-3])
        with pytest.raises(RuntimeError, match=r"\(-1\).*truncated"):
            r.ld.load_vocabulary(cut)
        assert r.ld.size(0) == 3
        check_result(r.ld.detect([frames[3]], [3])[0], want[3])          # the old vocabulary and the database stand
        r.ld.load_vocabulary(path)                                        # the same vocabulary from its file: the database is empty again
        assert r.ld.size(0) == 0
        for i in range(3):
            check_result(r.ld.detect([frames[i]], [i])[0], want[i])
            check_bag(r.ld, 0, i, entries[i])
