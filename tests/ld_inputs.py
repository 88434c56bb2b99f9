"""Inputs of the loop detector tests: generated vocabularies (the reference's brief_k10L6.bin is not available), irregular trees
for the descent, and the 85-keyframe sequence that reaches every branch of detectLoop."""
import functools

import numpy as np

from vplines_slam_amd.frontend import Vocabulary, TF_IDF

import ld_ref

M64 = (1 << 64) - 1


def to_words(x):
    """256-bit integer -> four 64-bit words"""
    return [x & M64, x >> 64 & M64, x >> 128 & M64, x >> 192 & M64]


def rand_desc(rng):
    return int.from_bytes(rng.bytes(32), "little")


def flip(x, n, rng):
    for b in rng.choice(256, n, replace=False):
        x ^= 1 << int(b)
    return x


def regular_vocabulary(k, L, seed, weighting=TF_IDF, stop_fraction=0.02, flips=(0, 48, 24, 12, 8, 6), shuffle=False):
    """A k-ary tree of L levels, numbered breadth first.  A child's descriptor is its parent's with flips[level - 1] bits turned
    (level 1: random), so a leaf's descriptor, and a slightly disturbed copy of it, descends to that leaf.  Leaf weights are
    log-uniform in [0.01, 10], a few of them 0 (stop words); inner weights 0 as DBoW2 leaves them."""
    rng = np.random.default_rng(seed)
    node_id, parent_id, weight, desc = [], [], [], []
    level_nodes, level_desc, nxt = [0], [0], 1
    for lv in range(1, L + 1):
        nn, nd = [], []
        for p, pd in zip(level_nodes, level_desc):
            for _ in range(k):
                d = rand_desc(rng) if lv == 1 else flip(pd, flips[min(lv - 1, len(flips) - 1)], rng)
                node_id.append(nxt); parent_id.append(p); desc.append(d)
                if lv == L:
                    weight.append(0.0 if rng.random() < stop_fraction else float(np.exp(rng.uniform(np.log(0.01), np.log(10.0)))))
                else:
                    weight.append(0.0)
                nn.append(nxt); nd.append(d)
                nxt += 1
        level_nodes, level_desc = nn, nd
    word_node = np.array(level_nodes)
    word_id = rng.permutation(len(word_node))
    order = rng.permutation(len(node_id)) if shuffle else np.arange(len(node_id))
    # (shuffled: the children of a node then stand in another order, and it is the file order that counts)
    D = np.array([to_words(d) for d in desc], np.uint64)
    return Vocabulary(k, L, np.array(node_id)[order], np.array(parent_id)[order], np.array(weight)[order], D[order], word_node, word_id,
                      weighting=weighting)


def leaf_descriptors(voc):
    """{word id: descriptor as a 256-bit integer}"""
    at = {int(n): i for i, n in enumerate(voc.node_id)}
    return {int(w): ld_ref.as_int(voc.descriptor[at[int(n)]]) for n, w in zip(voc.word_node, voc.word_id)}


# ---- the sequence: 85 keyframes, 70 places and then places 5 .. 19 again ----
SEQ_K, SEQ_L, SEQ_PER_FRAME, SEQ_FLIPS = 10, 4, 32, 4
SEQ_POOL = 3000          # the places draw their words from this many: two unrelated places share one or two, at small scores
SEQ_PLACES = list(range(70)) + list(range(5, 20))


@functools.lru_cache(maxsize=None)
def sequence_vocabulary():
    return regular_vocabulary(SEQ_K, SEQ_L, seed=20240611)


@functools.lru_cache(maxsize=None)
def sequence(seed=7, shift=0):
    """per keyframe a [32][4] uint64 array.  A place owns 32 descriptors (leaf descriptors of the vocabulary, drawn
    from a pool of SEQ_POOL words so that unrelated places share a word now and then).  A frame shows the
    first 16 of its place and the first 16 of its predecessor's place -- except at places divisible by 3, which show all 32 of
    their own -- each with SEQ_FLIPS bits turned.  shift: another sequence of the same shape (other places, other noise)."""
    voc = sequence_vocabulary()
    leaves = leaf_descriptors(voc)
    rng = np.random.default_rng(seed + 1000 * shift)
    pool = rng.permutation(len(leaves))[:SEQ_POOL]
    own = {p: [leaves[int(w)] for w in rng.choice(pool, SEQ_PER_FRAME, replace=False)] for p in range(70)}
    frames, prev = [], None
    for p in SEQ_PLACES:
        half = SEQ_PER_FRAME // 2
        base = own[p] if (p % 3 == 0 or prev is None) else own[prev][:half] + own[p][:half]
        frames.append(np.array([to_words(flip(d, SEQ_FLIPS, rng)) for d in base], np.uint64))
        prev = p
    return frames


@functools.lru_cache(maxsize=None)
def sequence_reference(seed=7, shift=0, first_index=0):
    """ld_ref on the sequence: (results per keyframe, the stored bags)"""
    det = ld_ref.Detector(sequence_vocabulary())
    res = [det.detect(f, first_index + i) for i, f in enumerate(sequence(seed, shift))]
    return res, det.entries


# ---- irregular trees for the descent ----
def tree_vocabulary(parents, descs, weights=None, weighting=TF_IDF, order=None, k=0, L=0):
    """parents[i], descs[i] (256-bit integers) of node i + 1; every leaf gets a word in node order (weight i + 1 unless given)"""
    n = len(parents)
    inner = set(parents)
    leaves = [i + 1 for i in range(n) if i + 1 not in inner]
    weights = [float(i + 1) for i in range(n)] if weights is None else weights
    order = list(range(n)) if order is None else order
    D = np.array([to_words(d) for d in descs], np.uint64).reshape(-1, 4)
    ids = np.arange(1, n + 1)
    return Vocabulary(k, L, ids[order], np.array(parents, np.int64)[order], np.array(weights, np.float64)[order], D[order], leaves,
                      np.arange(len(leaves)), weighting=weighting)


def irregular_tree(seed=3):
    """One tree with: a node with 1 child, a node with 17 children, leaves at depths 1 and 5, two children with equal descriptors,
    and a probe that is equidistant from two children.  Children lie near their parents, so a probe made from a node enters that
    node's branch.  Returns (parents, descriptors) for tree_vocabulary, {name: probe descriptor} and the node numbers by role."""
    rng = np.random.default_rng(seed)
    parents, descs = [], []

    def node(parent, d):
        parents.append(parent); descs.append(d)
        return len(parents)

    a = node(0, rand_desc(rng))           # 1: a leaf at depth 1
    b = node(0, rand_desc(rng))           # 2: one child, and so on down to depth 5
    c = node(0, rand_desc(rng))           # 3: 17 children
    e = node(0, rand_desc(rng))           # 4: two children with EQUAL descriptors
    g = node(0, rand_desc(rng))           # 5: two children at equal distance from a probe
    chain = b
    for _ in range(4):
        chain = node(chain, rand_desc(rng))          # depths 2 .. 5, one child each
    wide = [node(c, flip(descs[c - 1], 30, rng)) for _ in range(17)]
    same = flip(descs[e - 1], 20, rng)
    twins = [node(e, same), node(e, same)]
    base = flip(descs[g - 1], 20, rng)
    eq = [node(g, base ^ 0b01), node(g, base ^ 0b10)]     # the probe `base` is 1 bit from each
    probes = {"depth1": descs[a - 1], "chain": descs[b - 1], "wide_last": flip(descs[wide[16] - 1], 3, rng),
              "wide_first": flip(descs[wide[0] - 1], 3, rng), "twins": flip(same, 2, rng), "equidistant": base}
    notes = dict(a=a, chain_leaf=chain, wide=wide, twins=twins, eq=eq)
    return parents, descs, probes, notes
