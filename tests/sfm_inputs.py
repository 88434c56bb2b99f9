"""Inputs of the initial-structure tests: sequences from test_gpu_sequence.Measurements (a point cloud and per-frame observations)
as the feature manager and the image frames hold them when Estimator::initialStructure runs.  Tracks have mixed starts and lengths;
some have one observation and are never triangulated, some are seen in neither frame l nor frame 10 and get their position in
step 5.  relative_R / relative_T come from the true poses, relative_T of unit length as recoverPose gives it.  Observations are
exact, or carry a fixed-seed noise of half a pixel at f = 460.  Computed once per argument set and shared; nothing writes into what
is returned."""
import functools

import numpy as np

from test_gpu_sequence import quat_R, expso3
from init_align_inputs import measurements, KEY11, KEY14, KEY40   # noqa: F401

NF = 11
SIGMA = 0.5 / 460.0
ID0 = 1000


PATH_FRAMES = 14      # the stretch of the trajectory every sequence covers: over more frames no point stays in view


def logso3(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return w if th < 1e-9 else w * th / np.sin(th)


def cameras(M, F):
    """(R [F, 3, 3] camera to world, t [F, 3]) of the image frames: the true frames of M, or -- more image frames than M has -- F
    poses spread evenly over its path, interpolated between its frames"""
    ric, tic = quat_R(M.ex[3:]), M.ex[:3]
    n = len(M.pose_true)
    R0 = np.stack([quat_R(M.pose_true[f][3:]) @ ric for f in range(n)])
    t0 = np.stack([M.pose_true[f][:3] + quat_R(M.pose_true[f][3:]) @ tic for f in range(n)])
    if F <= n:
        return R0[:F], t0[:F]
    R, t = [], []
    for f in range(F):
        tau = f * (n - 1) / (F - 1)
        a = min(int(tau), n - 2)
        s = tau - a
        R.append(R0[a] @ expso3(s * logso3(R0[a].T @ R0[a + 1])))
        t.append((1 - s) * t0[a] + s * t0[a + 1])
    return np.stack(R), np.stack(t)


def visible(R, t, X):
    """the points in front of a camera with a 90 degree field of view"""
    pc = (X - t) @ R
    return set(np.nonzero((pc[:, 2] > 0.5) & (np.abs(pc[:, 0]) <= pc[:, 2]) & (np.abs(pc[:, 1]) <= pc[:, 2]))[0].tolist())


def project(R, t, X):
    pc = (X - t) @ R
    return pc[:2] / pc[2]


@functools.lru_cache(maxsize=None)
def sequence(F, key, l, noisy=False, n_tracks=70, seed=77, track_seed=3, starve=None, frame_starve=None):
    """-> (S, truth).  S: the dict tests/sfm_ref.initial_structure and capi.SfmInput take.  truth: c_q-free ground truth in the
    gauge of construct -- cam_R [11, 3, 3] / cam_t [11, 3] (world of frame l's camera -> camera i, lengths in units of the distance
    between the cameras of frames l and 10) and points [N, 3].
    starve = (window frame, k): the PnP of that frame -- l + 1, or a frame before l -- sees k points;
    frame_starve = (image frame, k): that non-key frame lists only k tracked points."""
    M = measurements(min(F, PATH_FRAMES), seed)
    rng = np.random.default_rng([track_seed, F, l])
    Rc, tc = cameras(M, F)
    key = list(key)
    seen_in = [visible(Rc[f], tc[f], M.pts) for f in range(F)]
    vis = [seen_in[key[i]] for i in range(NF)]
    # candidate points: seen in at least two consecutive window frames
    runs = {}
    for p in sorted(set.union(*vis)):
        best, a = (0, 0), None
        for i in range(NF + 1):
            inside = i < NF and p in vis[i]
            if inside and a is None:
                a = i
            if not inside and a is not None:
                if i - a > best[1] - best[0]:
                    best = (a, i)
                a = None
        if best[1] - best[0] >= 2:
            runs[p] = best
    full = [p for p, (a, b) in runs.items() if a == 0 and b == NF]
    assert len(full) >= 24, ("points seen all along", len(full))
    order = list(rng.permutation(sorted(runs)))
    picked, start, nobs = [], [], []
    # two dozen tracks over the whole window (every PnP of the chain sees at least ten), the rest cut at random
    for p in rng.permutation(full)[:24]:
        picked.append(int(p))
        a, b = runs[int(p)]
        start.append(a)
        nobs.append(b - a)
    for p in order:
        if len(picked) >= n_tracks:
            break
        if int(p) in picked:
            continue
        a, b = runs[int(p)]
        kind = len(picked) % 4
        if kind == 0:                              # one observation: never triangulated
            s, n = int(rng.integers(a, b)), 1
        elif kind == 1:                            # neither l nor frame 10, where the run allows it
            lo = max(a, l + 1) if l + 3 <= min(b, NF - 1) else a
            hi = min(b, NF - 1)
            if hi - lo < 2:
                lo, hi = a, b
            s = int(rng.integers(lo, hi - 1))
            n = int(rng.integers(2, hi - s + 1))
        else:
            s = int(rng.integers(a, b - 1))
            n = int(rng.integers(2, b - s + 1))
        picked.append(int(p))
        start.append(s)
        nobs.append(n)
    perm = rng.permutation(len(picked))
    picked, start, nobs = [picked[k] for k in perm], np.array([start[k] for k in perm]), np.array([nobs[k] for k in perm])
    if starve is not None:
        # The PnP of frame l + 1 sees the tracks that cover l .. 10, the PnP of a frame f < l those that cover f .. l.
        f, k = starve
        assert f == l + 1 or f < l
        lo, hi = (l, NF - 1) if f > l else (f, l)
        cover = [j for j in range(len(picked)) if start[j] <= lo and hi < start[j] + nobs[j]]
        for j in cover[k:]:
            if f > l:                              # the track ends in frame 9
                nobs[j] = NF - 1 - start[j]
            else:                                  # the track starts behind f
                nobs[j] -= f + 1 - start[j]
                start[j] = f + 1
    noise = np.random.default_rng([seed, 99]).normal(0, SIGMA, (len(M.pts), F, 2))

    def uv(p, f):
        x = project(Rc[f], tc[f], M.pts[p])
        return x + noise[p, f] if noisy else x

    obs = np.array([uv(p, key[s + k]) for p, s, n in zip(picked, start, nobs) for k in range(n)])
    ids = np.array([ID0 + p for p in picked])
    frame_pts = {}
    for f in range(F):
        if f in key:
            continue
        seen = [p for p in picked if p in seen_in[f]]
        others = [p for p in sorted(seen_in[f]) if p not in picked][:5]           # ids the SfM never saw
        if frame_starve is not None and frame_starve[0] == f:
            sch = _tracked(l, start, nobs)
            seen = [p for p in seen if sch[picked.index(p)]][:frame_starve[1]] + [p for p in seen if not sch[picked.index(p)]]
        lst = list(rng.permutation(seen + others))
        frame_pts[f] = (np.array([ID0 + p for p in lst]), np.array([uv(p, f) for p in lst]).reshape(-1, 2))
    kl, k10 = key[l], key[NF - 1]
    base = np.linalg.norm(tc[k10] - tc[kl])
    S = dict(n_frames=F, key=np.array(key), l=l, relative_R=Rc[kl].T @ Rc[k10], relative_T=Rc[kl].T @ (tc[k10] - tc[kl]) / base,
             ric=quat_R(M.ex[3:]), track_id=ids, track_start=start, track_nobs=nobs, track_obs=obs, frame_pts=frame_pts)
    truth = dict(cam_R=np.stack([Rc[key[i]].T @ Rc[kl] for i in range(NF)]),
                 cam_t=np.stack([Rc[key[i]].T @ (tc[kl] - tc[key[i]]) / base for i in range(NF)]),
                 points=np.stack([Rc[kl].T @ (M.pts[p] - tc[kl]) / base for p in picked]), base=base,
                 img_R=np.stack([Rc[kl].T @ Rc[f] for f in range(F)]), img_T=np.stack([Rc[kl].T @ (tc[f] - tc[kl]) / base for f in range(F)]))
    return S, truth


def _tracked(l, start, nobs):
    import sfm_ref
    return sfm_ref.schedule(l, start, nobs)["step"] >= 0


def random_tables(rng, n):
    """n random tracks inside the window, start + nobs <= 11: half of them anywhere, half over most of the window"""
    long_ = rng.random(n) < 0.5
    start = np.where(long_, rng.integers(0, 3, n), rng.integers(0, NF, n))
    nobs = np.array([int(rng.integers(NF - s - 2, NF - s + 1)) if g else int(rng.integers(1, NF - s + 1)) for s, g in zip(start, long_)], dtype=np.int64)
    return start, nobs


# The sequences the GPU tests solve (tests/test_gpu_init_structure.py); test_sfm_reference.py checks that the float64 and the
# extended-precision run of the restatement take the same decisions on every one of them.
CASES = {
    "F11 l4 exact": dict(F=11, key=KEY11, l=4),
    "F11 l4 noisy": dict(F=11, key=KEY11, l=4, noisy=True),
    "F11 l0 noisy": dict(F=11, key=KEY11, l=0, noisy=True),
    "F11 l9 exact": dict(F=11, key=KEY11, l=9),
    "F14 l4 exact": dict(F=14, key=KEY14, l=4),
    "F14 l6 noisy": dict(F=14, key=KEY14, l=6, noisy=True),
    "F40 l5 exact": dict(F=40, key=KEY40, l=5),
    "F40 l3 noisy": dict(F=40, key=KEY40, l=3, noisy=True),
    "F11 l4 noisy, frame 5 starved": dict(F=11, key=KEY11, l=4, noisy=True, starve=(5, 9)),
    "F11 l4 noisy, frame 2 starved": dict(F=11, key=KEY11, l=4, noisy=True, starve=(2, 9)),
    "F14 l4 noisy, image frame 7 starved": dict(F=14, key=KEY14, l=4, noisy=True, frame_starve=(7, 5)),
}


def case(name):
    return sequence(**CASES[name])


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's float64 and extended-precision runs of a case"""
    import sfm_ref
    sfm_ref.require_extended()
    S, _ = case(name)
    return sfm_ref.initial_structure(S, np.float64), sfm_ref.initial_structure(S, np.longdouble)
