"""Seeded inputs of test_preint_reference.py and test_gpu_preint.py: single intervals (`cases`) from a smooth true motion plus
noise, and the batches vpl_preintegrate_batch is called with (`batches`, `position_batches`, `nan_row_batch`).

Every case but `default20` uses four noise densities that differ by orders of magnitude (NOISE), so that a swap of two of them
or a lost factor moves an entry of P by far more than its unit.  In every batch offset[k] + max(nsamples[k], 1) stays within
the rows the call uploads (those below max(offset + nsamples)): no implementation, whether or not it reads a row for an empty
interval, is led outside an allocation."""
import functools

import numpy as np

import vplines_slam_amd as v

NOISE = (0.2, 0.003, 4e-4, 7e-6)            # acc_n, gyr_n, acc_w, gyr_w
BA_BIG, BG_BIG = np.array([0.31, -0.28, 0.27]), np.array([-0.06, 0.05, 0.062])      # |ba| ~ 0.5, |bg| ~ 0.1
ZERO = np.zeros(3)


def default_noise():
    o = v.default_options()
    return (o.acc_n, o.gyr_n, o.acc_w, o.gyr_w)


# ---- motions: t [n] -> (acc [n, 3], gyr [n, 3]), smooth in t -------------------------------------------------------------
def gentle(t, ph=0.0):
    acc = np.stack([0.6 * np.sin(1.3 * t + ph) + 0.2, -0.4 * np.cos(0.9 * t + ph), 9.8 + 0.3 * np.sin(2.1 * t)], axis=-1)
    gyr = np.stack([0.3 * np.cos(1.1 * t + ph), -0.2 * np.sin(1.7 * t), 0.25 * np.sin(0.8 * t + 0.4 + ph)], axis=-1)
    return acc, gyr


def fast(t, ph=0.0):
    """10 rad/s with 30 m/s^2: at dt = 5 ms the un-normalised (1, w dt / 2) is 3e-4 off unit length"""
    acc = np.stack([27.0 * np.cos(3.0 * t + ph), -18.0 * np.sin(2.0 * t + 0.3), 9.8 + 15.0 * np.sin(4.0 * t + ph)], axis=-1)
    gyr = np.stack([6.0 * np.cos(2.0 * t + ph), 5.5 * np.sin(3.0 * t + 1.0), -5.8 * np.cos(1.5 * t + 0.2)], axis=-1)
    return acc, gyr


def pure_rotation(t, ph=0.0):
    """about a fixed axis at 2 rad/s, no translation: the accelerometer sees gravity turning in the body frame"""
    th = 2.0 * t + ph
    acc = 9.81 * np.stack([np.sin(th) * 0.6, np.sin(th) * 0.8, np.cos(th)], axis=-1)
    gyr = np.stack([1.6 + 0 * t, -1.2 + 0 * t, 0 * t], axis=-1)
    return acc, gyr


def _case(motion, dts, ba, bg, seed, noise=NOISE, sigma=(0.05, 0.002), exact_acc=None):
    """an interval: the measurement before it at t = 0, sample k at t_k = sum dts[:k + 1]; white noise of `sigma` on top"""
    rng = np.random.default_rng(seed)
    dts = np.asarray(dts, np.float64)
    t = np.concatenate([[0.0], np.cumsum(dts)])
    acc, gyr = motion(t)
    acc = acc + sigma[0] * rng.normal(size=acc.shape) + ba
    gyr = gyr + sigma[1] * rng.normal(size=gyr.shape) + bg
    if exact_acc is not None:
        acc[:] = exact_acc
    samples = np.concatenate([dts[:, None], acc[1:], gyr[1:]], axis=1).reshape(-1, 7)
    return dict(samples=samples, acc0=acc[0].copy(), gyr0=gyr[0].copy(), ba=np.array(ba, np.float64), bg=np.array(bg, np.float64),
                noise=tuple(noise))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(samples [n, 7], acc0, gyr0, ba, bg, noise).  Sample counts 0, 1, 2, 3, 19, 20, 37, 64; dt 5 ms and 2.5 ms,
    jittered 1 .. 9 ms, one dt == 0 mid-interval, 64 samples over more than 10 s; biases zero and (|ba| ~ 0.5, |bg| ~ 0.1);
    gentle, fast (10 rad/s, 30 m/s^2 at 5 ms), pure rotation, free fall (acc == ba exactly: both skews are all zeros)"""
    rng = np.random.default_rng(4242)
    reg = lambda n, dt: np.full(n, dt)
    c = {}
    c["n0"] = _case(gentle, reg(0, 0.005), BA_BIG, BG_BIG, 1)
    c["n1"] = _case(gentle, reg(1, 0.005), ZERO, ZERO, 2)
    c["n2"] = _case(gentle, reg(2, 0.0025), BA_BIG, BG_BIG, 3)
    c["n3"] = _case(gentle, reg(3, 0.005), ZERO, ZERO, 4)
    c["n19"] = _case(gentle, reg(19, 0.0025), ZERO, ZERO, 5)
    c["n20"] = _case(gentle, reg(20, 0.005), BA_BIG, BG_BIG, 6)
    c["n37_jitter"] = _case(gentle, rng.uniform(0.001, 0.009, 37), BA_BIG, BG_BIG, 7)
    c["n64"] = _case(gentle, reg(64, 0.0025), ZERO, ZERO, 8)
    dts = reg(20, 0.005)
    dts[10] = 0.0
    c["n20_dt0"] = _case(gentle, dts, BA_BIG, BG_BIG, 9)
    c["n64_long"] = _case(gentle, rng.uniform(0.15, 0.19, 64), ZERO, ZERO, 10)
    c["n20_fast"] = _case(fast, reg(20, 0.005), BA_BIG, BG_BIG, 11)
    c["n64_fast"] = _case(fast, reg(64, 0.005), ZERO, ZERO, 12)
    c["n37_rot"] = _case(pure_rotation, reg(37, 0.005), BA_BIG, BG_BIG, 13)
    c["n20_fall"] = _case(gentle, reg(20, 0.005), BA_BIG, BG_BIG, 14, exact_acc=BA_BIG)
    c["n3_fast_jitter"] = _case(fast, rng.uniform(0.001, 0.009, 3), BA_BIG, BG_BIG, 15)
    c["default20"] = _case(gentle, reg(20, 0.005), BA_BIG, BG_BIG, 16, noise=default_noise())
    return c


COUNTS = dict(n0=0, n1=1, n2=2, n3=3, n19=19, n20=20, n37_jitter=37, n64=64, n20_dt0=20, n64_long=64, n20_fast=20, n64_fast=64,
              n37_rot=37, n20_fall=20, n3_fast_jitter=3, default20=20)
DISTINCT = [k for k in COUNTS if k != "default20"]


# ---- one continuous motion at dt, dt / 2, dt / 4 over the same span (checks (a) and (b)) ----------------------------------
def _halving(motion, span, n0, ba, bg):
    out = []
    for n in (n0, 2 * n0, 4 * n0):
        out.append(_case(motion, np.full(n, span / n), ba, bg, 0, sigma=(0.0, 0.0)))
    return out


@functools.lru_cache(maxsize=None)
def halving():
    """check (a): the fast motion over 0.16 s at dt = 10, 5, 2.5 ms, linearised at the large biases"""
    return _halving(fast, 0.16, 16, BA_BIG, BG_BIG)


@functools.lru_cache(maxsize=None)
def halving_noise():
    """check (b): intervals of 4, 8, 16 samples of the fast motion over 0.08 s (dt = 20, 10, 5 ms)"""
    return _halving(fast, 0.08, 4, BA_BIG, BG_BIG)


# ---- batches --------------------------------------------------------------------------------------------------------------
def assemble(names, storage=None, gap=0, empty_at=0, fill=np.nan):
    """the arrays of one vpl_preintegrate_batch call over the cases `names`.  The samples of the intervals are stored in the order
    `storage` (a permutation of range(len(names)); default: as listed), each followed by `gap` rows of `fill` that belong to no
    interval; one more such row ends the array.  An empty interval's offset is `empty_at` (< 0: counted from the end, -1 = the
    final fill row).  -> (offset, nsamples, samples, acc0, gyr0, ba, bg)"""
    cs = [cases()[k] for k in names]
    storage = list(range(len(names))) if storage is None else list(storage)
    assert sorted(storage) == list(range(len(names)))
    rows, offset = [], [0] * len(names)
    at = 0
    for i in storage:
        s = cs[i]["samples"]
        offset[i] = at
        rows.append(s)
        rows.append(np.full((gap, 7), fill))
        at += len(s) + gap
    rows.append(np.full((1, 7), fill))
    samples = np.ascontiguousarray(np.concatenate(rows, axis=0))
    total = len(samples)
    nsamples = [len(c["samples"]) for c in cs]
    for i, n in enumerate(nsamples):
        if n == 0:
            offset[i] = empty_at % total
    # vpl_preintegrate_batch uploads the rows below max(offset + nsamples): an empty interval's row has to lie among THEM to be
    # a row the device holds (a batch of empty intervals only uploads nothing, and nothing is read)
    uploaded = max(o + n for o, n in zip(offset, nsamples))
    for i, n in enumerate(nsamples):
        assert 0 <= offset[i] and offset[i] + max(n, 1) <= (uploaded if uploaded else total)
    st = lambda k: np.ascontiguousarray(np.stack([c[k] for c in cs]))
    return (np.array(offset, np.int32), np.array(nsamples, np.int32), samples, st("acc0"), st("gyr0"), st("ba"), st("bg"))


def batches():
    """name -> (names of the intervals, arrays): n = 1, 4, 5, 7, 15; a block of lengths (0, 1, 37, 3); mixed lengths in every
    block; offsets not monotone with rows between the intervals that belong to nobody; the case at the default options alone.
    The empty intervals point at a finite row of another interval here (the NaN row is nan_row_batch's)"""
    b = {}
    b["one"] = ["n20"]
    b["default"] = ["default20"]
    b["block_0_1_37_3"] = ["n0", "n1", "n37_jitter", "n3"]
    b["five"] = ["n19", "n2", "n64", "n20_fast", "n20_dt0"]
    b["seven"] = ["n64_long", "n1", "n20_fall", "n3_fast_jitter", "n37_rot", "n0", "n20"]
    b["all"] = list(DISTINCT)
    out = {k: (names, assemble(names, fill=0.5)) for k, names in b.items()}
    rng = np.random.default_rng(99)
    out["scattered"] = (b["all"], assemble(b["all"], storage=rng.permutation(len(b["all"])), gap=2, empty_at=5, fill=0.5))
    return out


SUBJECT = "n20"


def position_batches():
    """[(names, arrays, index of SUBJECT)]: the same interval in groups 0..3 of a block beside neighbours of every other length,
    alone (n = 1), as the only live group of a second block (n = 5), in n = 7, and with its samples stored last, first and between"""
    others = ["n0", "n1", "n64", "n37_jitter", "n3", "n19", "n2", "n64_long", "n20_fast"]
    out = []
    for g in range(4):
        names = [others[(3 * g + k) % len(others)] for k in range(3)]
        names.insert(g, SUBJECT)
        out.append((names, assemble(names, storage=np.roll(np.arange(4), g), gap=g, fill=0.5), g))
    out.append(([SUBJECT], assemble([SUBJECT], fill=0.5), 0))
    names = others[2:6] + [SUBJECT]
    out.append((names, assemble(names, storage=[4, 0, 1, 2, 3], fill=0.5), 4))
    names = others[3:6] + others[0:2] + [SUBJECT] + others[6:7]
    out.append((names, assemble(names, storage=[6, 0, 5, 1, 2, 3, 4], gap=1, fill=0.5), 5))
    return out


def nan_row_batch():
    """(names, arrays, index of the empty interval): lengths (20, 0, 3, 37), one row of NaN that belongs to nobody behind each
    interval's samples; the empty interval's offset is the first of them, row 20 -- below max(offset + nsamples), so uploaded"""
    names = ["n20", "n0", "n3", "n37_jitter"]
    arr = assemble(names, gap=1, empty_at=20, fill=np.nan)
    off, ns, smp = arr[0], arr[1], arr[2]
    owned = np.zeros(len(smp), bool)
    for o, n in zip(off, ns):
        owned[o:o + n] = True
    assert off[1] == 20 and not owned[20] and np.all(np.isnan(smp[20])) and np.isfinite(smp[owned]).all()
    assert 20 < max(o + n for o, n in zip(off, ns))
    return names, arr, 1
