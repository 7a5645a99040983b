"""The definition of the device input sampler (csrc/input_stage.hip, ``prcnn_input_stage``): numpy, no torch, no GPU.

Given the class of every raw point (0 = invalid, 1 = near, 2 = far) and the 64-bit seed, every output row of the stage is
determined.  This file states that rule; tests/test_gpu_input_stage.py holds the kernel to it pick for pick, and
tests/test_input_stage_ref.py checks the rule against itself.  All hash arithmetic is uint32, modulo 2^32.

  fmix32        the murmur3 finaliser, a bijection of the 32-bit words
  seed words    sa = fmix32(seed & 0xffffffff), sb = fmix32((seed >> 32) ^ 0x9e3779b9), sc = sa ^ 0x7f4a7c15
  selection key of raw index i: fmix32(i ^ sa); "the k smallest of a set" is by this key (keys are distinct)

  no valid point          every row -1
  n_valid > npoints       far_keep = min(n_far, npoints_faraway, npoints); taken = the far_keep smallest far points and the
                          min(n_near, npoints - far_keep) smallest near points; if that is short of npoints, the rest are
                          copies drawn with replacement, from the near class if it has a point, else from any taken point
  n_valid <= npoints      taken = every valid point, extra = npoints - n_valid; 0 < extra <= n_valid: the extras are the
                          ``extra`` smallest valid points, each once more; otherwise copies with replacement from any taken point
  nothing taken           (npoints_faraway = 0, more than npoints valid points, all far) the empty scene again: every row -1
  copy e                  h = fmix32(e ^ sc); the pick is the taken point of rank h % have in ASCENDING RAW INDEX; while the pool
                          is one class and the pick is of the other, h = fmix32(h + 0x632be5ab) and pick again; after 16
                          re-draws the last pick stands
  shuffle                 every entry carries a key -- a taken point fmix32(i ^ sb), a distinct extra fmix32(i ^ sc), a copy
                          fmix32(h ^ sb ^ 0x51ed270b) with its final h -- and the output is the entries sorted by (key, raw index)

The loader's seeds are ``seed + scene id``, below 2^32, so sb is ONE constant there: the relative output order of two taken raw
indices is the same in every scene and every run.  That is part of the definition (the driver's dumped detections depend on it).

``sample_choice(..., trace=set())`` also records which branches the cloud took, under the names of ``BRANCHES``."""
import numpy as np

_M32 = np.uint64(0xffffffff)

BRANCHES = ("empty", "nothing_taken", "far_by_threshold", "far_whole", "far_none", "near_by_threshold", "near_exact", "near_none",
            "near_copies", "any_copies_large", "exact", "distinct_extras", "distinct_all", "any_copies_small", "redraw", "fallback16")


def fmix32(h):
    """murmur3's 32-bit finaliser on an integer or an array of them -> uint64 holding 32-bit words"""
    h = np.asarray(h).astype(np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & _M32
    return h ^ (h >> np.uint64(16))


def seed_words(seed):
    seed = int(seed) & (2 ** 64 - 1)
    sa = int(fmix32(seed & 0xffffffff))
    sb = int(fmix32((seed >> 32) ^ 0x9e3779b9))
    return sa, sb, sa ^ 0x7f4a7c15


def selection_keys(n, seed):
    """key of every raw index 0 .. n-1"""
    return fmix32(np.arange(n, dtype=np.uint64) ^ np.uint64(seed_words(seed)[0]))


def sample_choice(cls, npoints, npoints_faraway, seed, trace=None):
    """cls (n,) in {0, 1, 2} -> choice (npoints,) int64: the raw index of every output row, -1 in all rows of an empty scene"""
    cls = np.asarray(cls)
    trace = set() if trace is None else trace
    sa, sb, sc = (np.uint64(w) for w in seed_words(seed))
    idx = np.arange(len(cls), dtype=np.uint64)
    key = fmix32(idx ^ sa)
    near, far = idx[cls == 1], idx[cls == 2]
    valid = idx[cls != 0]
    empty = np.full(npoints, -1, dtype=np.int64)

    def smallest(ids, k):
        return ids[np.argsort(key[ids.astype(np.int64)], kind="stable")[:k]]

    if len(valid) == 0:
        trace.add("empty")
        return empty
    distinct = idx[:0]
    pool_cls = 0
    if len(valid) > npoints:
        far_keep = min(len(far), npoints_faraway, npoints)
        near_keep = min(len(near), npoints - far_keep)
        taken = np.concatenate([smallest(far, far_keep), smallest(near, near_keep)])
        copies = npoints - len(taken)
        trace.add("far_none" if far_keep == 0 else "far_by_threshold" if far_keep < len(far) else "far_whole")
        if copies:
            pool_cls = 1 if len(near) else 0
            trace.add("near_copies" if pool_cls else "any_copies_large")
        else:
            trace.add("near_none" if near_keep == 0 else "near_by_threshold" if near_keep < len(near) else "near_exact")
    else:
        taken = valid
        copies = npoints - len(valid)
        if copies == 0:
            trace.add("exact")
        elif copies <= len(valid):
            distinct, copies = smallest(valid, copies), 0
            trace.add("distinct_all" if len(distinct) == len(valid) else "distinct_extras")
        else:
            trace.add("any_copies_small")
    if len(taken) == 0:
        trace.add("nothing_taken")
        return empty

    taken = np.sort(taken)                                   # rank = position in ascending raw index
    have = np.uint64(len(taken))
    h = fmix32(np.arange(copies, dtype=np.uint64) ^ sc)
    pick = taken[(h % have).astype(np.int64)]
    if pool_cls:
        for _ in range(16):
            other = cls[pick.astype(np.int64)] != pool_cls
            if not other.any():
                break
            trace.add("redraw")
            h[other] = fmix32(h[other] + np.uint64(0x632be5ab))
            pick[other] = taken[(h[other] % have).astype(np.int64)]
        if (cls[pick.astype(np.int64)] != pool_cls).any():
            trace.add("fallback16")
    rows = np.concatenate([taken, distinct, pick])
    keys = np.concatenate([fmix32(taken ^ sb), fmix32(distinct ^ sc), fmix32(h ^ sb ^ np.uint64(0x51ed270b))])
    assert len(rows) == npoints
    return rows[np.lexsort((rows, keys))].astype(np.int64)


def classify(rect, scope, far_depth):
    """rect (n, 3) f32 in the rect frame, no image filter -> cls (n,) uint8.  The f32 coordinates are compared with the f64 scope
    (3, 2) in double -- f32(70.4) > 70.4 is outside -- and near / far is z < f32(far_depth) in f32."""
    rect = np.asarray(rect, dtype=np.float32)
    r = rect.astype(np.float64)
    scope = np.asarray(scope, dtype=np.float64).reshape(3, 2)
    ok = np.ones(len(rect), dtype=bool)
    for a in range(3):
        ok &= (r[:, a] >= scope[a, 0]) & (r[:, a] <= scope[a, 1])
    return np.where(ok, np.where(rect[:, 2] < np.float32(far_depth), 1, 2), 0).astype(np.uint8)


SCOPE = np.array([[-40, 40], [-1, 3], [0, 70.4]], dtype=np.float64)      # config.PC_AREA_SCOPE
FAR_DEPTH = 40.0

# (near, far, invalid) at npoints = 256, npoints_faraway = 64 -> the branch names the cloud must reach
BRANCH_CASES = (
    ((1000, 200, 50), {"far_by_threshold", "near_by_threshold"}),
    ((1000, 64, 50), {"far_whole", "near_by_threshold"}),
    ((1000, 0, 50), {"far_none", "near_by_threshold"}),
    ((192, 500, 9), {"far_by_threshold", "near_exact"}),
    ((100, 500, 9), {"far_by_threshold", "near_copies", "redraw"}),
    ((3, 400, 0), {"far_by_threshold", "near_copies", "redraw", "fallback16"}),
    ((0, 500, 9), {"far_by_threshold", "any_copies_large"}),
    ((200, 56, 9), {"exact"}),
    ((255, 0, 3), {"distinct_extras"}),
    ((100, 28, 0), {"distinct_all"}),
    ((100, 27, 3), {"any_copies_small"}),
    ((1, 0, 5), {"any_copies_small"}),
    ((0, 1, 0), {"any_copies_small"}),
    ((0, 0, 7), {"empty"}),
    ((0, 0, 0), {"empty"}),
)


def make_cloud(n_near, n_far, n_invalid, rng):
    """A rect-frame cloud (n, 3) f32 whose classes are exact by construction: near points at z < 39.9, far ones at 40.1 <= z <= 70,
    invalid ones outside SCOPE on one axis, all interleaved at random."""
    near = rng.uniform([-40, -1, 0], [40, 3, 39.9], (n_near, 3))
    far = rng.uniform([-40, -1, 40.1], [40, 3, 70.0], (n_far, 3))
    bad = rng.uniform([-40, -1, 0], [40, 3, 70.0], (n_invalid, 3))
    axis = rng.integers(0, 3, n_invalid)
    outside = np.array([[-40.5, 41.0], [-1.25, 3.5], [-0.5, 70.5]])
    bad[np.arange(n_invalid), axis] = outside[axis, rng.integers(0, 2, n_invalid)]
    pts = np.concatenate([near, far, bad]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    cls = classify(pts, SCOPE, FAR_DEPTH)
    assert (int((cls == 1).sum()), int((cls == 2).sum()), int((cls == 0).sum())) == (n_near, n_far, n_invalid)
    return pts


def expected(rect, cls, npoints, npoints_faraway, seed, trace=None):
    """What the stage returns for one scene: (out (npoints, 3) f32, stats (3,) = #valid, #near, #far, choice (npoints,))"""
    cls = np.asarray(cls)
    choice = sample_choice(cls, npoints, npoints_faraway, seed, trace)
    rect = np.asarray(rect, dtype=np.float32)[:, :3]
    out = rect[choice] if choice[0] >= 0 else np.zeros((npoints, 3), dtype=np.float32)
    n_near, n_far = int((cls == 1).sum()), int((cls == 2).sum())
    return out, np.array([n_near + n_far, n_near, n_far], dtype=np.int32), choice
