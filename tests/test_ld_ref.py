"""tests/ld_ref.py, the restatement the loop detector is held to, against independent statements of the same thing; and the
85-keyframe sequence of tests/ld_inputs.py on the restatement's own output: it reaches every branch of detectLoop before any GPU
is involved.  No GPU."""
import collections

import numpy as np

from vplines_slam_amd.frontend import Vocabulary

import ld_inputs
import ld_ref


def test_score_is_one_minus_half_the_l1_distance():
    rng = np.random.default_rng(5)
    n_words = 40
    for _ in range(200):
        bags = []
        for _ in range(2):
            m = int(rng.integers(1, 25))
            words = sorted(int(w) for w in rng.choice(n_words, m, replace=False))
            vals = rng.uniform(0.01, 3.0, m)
            vals = (vals / vals.sum()).tolist()
            bags.append((words, vals))
        (qw, qv), (dw, dv) = bags
        got = ld_ref.query([(dw, dv)], qw, qv, 4, -1)
        v, w = np.zeros(n_words), np.zeros(n_words)
        v[qw], w[dw] = qv, dv
        if not set(qw) & set(dw):
            assert got == []
            continue
        assert len(got) == 1 and got[0][0] == 0
        assert abs(got[0][1] - (1.0 - 0.5 * np.abs(v - w).sum())) < 1e-12


def hand_vocabulary():
    """root -> 1, 2;  1 -> 3 (word 0, weight 0.5), 4 (word 1, 0.25);  2 -> 5 (word 2, weight 0: a stop word), 6 (word 3, 1.0)"""
    desc = {1: 0, 2: 0xFFFFFFFFFFFFFFFF, 3: 0, 4: 0xFF, 5: 0xFFFFFFFFFFFFFFFF, 6: 0xFFFFFFFFFFFF0000}
    ids = [1, 2, 3, 4, 5, 6]
    return Vocabulary(2, 2, ids, [0, 0, 1, 1, 2, 2], [0, 0, 0.5, 0.25, 0.0, 1.0], [ld_inputs.to_words(desc[i]) for i in ids],
                      [3, 4, 5, 6], [0, 1, 2, 3])


HAND_FRAME = [0x1, 0x3, 0xFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFF0000]


def test_hand_worked_case():
    tree = ld_ref.Tree(hand_vocabulary())
    descs = [ld_inputs.to_words(d) for d in HAND_FRAME]
    # 0x1: 1 bit from node 1 (63 from node 2), then 1 bit from node 3 (7 from node 4); 0x3 likewise: the same word twice
    # 0xFF: node 1 (8 against 56), node 4 exactly;  all ones: node 2, node 5 exactly: the stop word
    # the last: 48 bits from node 1, 16 from node 2; node 6 exactly
    assert [tree.descend(d) for d in descs] == [(0, 0.5), (0, 0.5), (1, 0.25), (2, 0.0), (3, 1.0)]
    words, values = tree.transform(descs)
    # word 0: 0.5 + 0.5, word 1: 0.25, word 3: 1.0; the norm 2.25
    assert words == [0, 1, 3]
    assert values == [0.4444444444444444, 0.1111111111111111, 0.4444444444444444]
    det = ld_ref.Detector(hand_vocabulary())
    first = det.detect(descs[2:], 0)                 # {1: 0.25, 3: 1.0} / 1.25, nothing stored before it
    assert first["ids"] == [] and det.entries[0] == ([1, 3], [0.2, 0.8])
    got = det.detect(descs, 1)
    # shared words 1 and 3: min(1/9, 0.2) + min(4/9, 0.8) = 5/9
    assert got["ids"] == [0] and got["n_words"] == 3 and got["entry"] == 1
    assert abs(got["scores"][0] - 0.5555555555555556) < 1e-15
    assert got["loop_index"] == -1


def test_binary_and_idf_set_a_weight_once():
    for weighting, want in ((ld_ref.TF_IDF, 1.0), (ld_ref.TF, 1.0), (ld_ref.IDF, 0.5), (ld_ref.BINARY, 0.5)):
        voc = hand_vocabulary()
        voc.weighting = weighting
        words, values = ld_ref.Tree(voc).transform([ld_inputs.to_words(d) for d in HAND_FRAME])
        norm = want + 0.25 + 1.0
        assert words == [0, 1, 3] and values == [want / norm, 0.25 / norm, 1.0 / norm]


def test_eligibility_is_taken_literally():
    det = ld_ref.Detector(hand_vocabulary())
    for _ in range(60):
        det.add([])
    assert det.eligible(48) == [59]                       # max_id -2: the newest only
    assert det.eligible(49) == list(range(60))            # max_id -1: all
    assert det.eligible(50) == [59]                       # max_id 0
    assert det.eligible(51) == [0, 59]                    # < 1, and the newest


def test_the_sequence_reaches_every_branch():
    res, entries = ld_inputs.sequence_reference()
    assert len(res) == len(entries) == 85 and [r["entry"] for r in res] == list(range(85))
    assert all(len(f) == ld_inputs.SEQ_PER_FRAME for f in ld_inputs.sequence())
    late = res[51:]
    assert sum(r["loop_index"] == -1 for r in late) >= 5 and sum(r["loop_index"] >= 0 for r in late) >= 5
    assert all(r["loop_index"] == -1 for r in res[:51])
    lengths = collections.Counter(len(r["ids"]) for r in res)
    assert set(lengths) == {0, 1, 2, 3, 4}, lengths
    first = [r["scores"][0] for r in res if r["scores"]]
    other = [s for r in res for s in r["scores"][1:]]
    assert sum(s > 0.05 for s in first) >= 5 and sum(s <= 0.05 for s in first) >= 5
    assert sum(s > 0.015 for s in other) >= 5 and sum(s <= 0.015 for s in other) >= 5
    # a loop names an old keyframe, never the neighbour; the replacement by a smaller id happens too
    assert all(r["loop_index"] < i - 50 for i, r in enumerate(res) if r["loop_index"] >= 0)
    assert any(r["loop_index"] >= 0 and r["loop_index"] != r["ids"][0] for r in res)
    assert any(r["loop_index"] >= 0 and r["loop_index"] == r["ids"][0] for r in res)
    # stop words are met, and words seen twice in one frame
    assert any(r["n_words"] < ld_inputs.SEQ_PER_FRAME for r in res)
