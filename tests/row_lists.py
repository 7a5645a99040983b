"""The row list of a ball query, as numpy: the DEFINITION every producer is compared with row for row (csrc/ball_pack.hip
ball_pack_kernel, ball_pack_count_kernel / ball_pack_write_kernel, csrc/roi_geometry.hip roi_pack_out), and seeded generators of
inputs that satisfy the contracts those kernels rely on.  numpy only: no GPU, no import of the package.

A row list holds the distinct (centre, point) pairs of an index tensor idx (b, m, nsample), per cloud in centre order, cut into
64-row tiles (include/prcnn_hip.h, prcnn_ball_pack / prcnn_ball_pack_rep / prcnn_ball_pack_ex).  Per cloud, lim = max(limit, 1), or
no bound without `limit`:

  without rep   cnt[c] = 1 + max{p > 0 : idx[c,p] != idx[c,0] and idx[c,p] < lim}, 1 if there is no such slot; row p < cnt[c] lists
                point k = idx[c,p] if idx[c,p] < lim, else idx[c,0]
  with rep      the kept slots are slot 0 and every p > 0 with idx[c,p] != idx[c,0], idx[c,p] < lim and rep[idx[c,p]] == idx[c,p],
                listed in slot order; cnt[c] = their number
  crep          cnt[c] = 0 where crep[c] != c
  a row         rowinfo = c << 16 | k, rowdxyz = (xyz[k] - new_xyz[c], 0): one f32 subtraction per component
  tiles         ceil(rows / 64) per cloud; the missing rows of the cloud's last tile are copies of (m-1) << 16 | idx[m-1,0] with that
                pair's relative coordinates -- also when centre m-1 has no rows of its own
  a list        the tiles of its clouds; hdr[0] = tiles, hdr[1] = rows, tilecloud[t] = the cloud's index inside the list
"""
import collections

import numpy as np

ROWS = 64            # rows per tile
CHUNK = 64           # centres per workgroup of the two-launch kernels (csrc/ball_pack.hip PK_CH): where tiles meet chunk boundaries
TWO_LAUNCH_M = 512   # !rep && m >= 512 takes the two-launch kernels

MUTANTS = ("pad_with_last_row", "ignore_limit", "rep_as_prefix", "ignore_crep")


class CloudRows(tuple):
    """(rowinfo u32[rows], rowdxyz f32[rows, 4], cnt i64[m]) of one cloud; .pad = (rowinfo word, rowdxyz[4]) of the padding row"""
    pad = None


def _cloud_rows(idx, xyz, new_xyz, limit, rep, crep, mutant):
    m, ns = idx.shape
    idx = idx.astype(np.int64)
    lim = max(int(limit), 1) if limit is not None and mutant != "ignore_limit" else np.iinfo(np.int64).max
    slot = np.arange(ns)
    ok = (idx != idx[:, :1]) & (idx < lim) & (slot > 0)
    if rep is not None:
        ok &= rep.astype(np.int64)[idx] == idx
    if rep is not None and mutant != "rep_as_prefix":
        keep = ok | (slot == 0)                                      # a mask: kept slots may sit anywhere in the row
        cnt = keep.sum(1)
    else:
        cnt = 1 + np.where(ok, slot, 0).max(1)                       # a prefix: up to the last slot that counts
        keep = slot[None, :] < cnt[:, None]
    if crep is not None and mutant != "ignore_crep":
        own = crep.astype(np.int64) == np.arange(m)
        cnt = np.where(own, cnt, 0)
        keep &= own[:, None]
    c, p = np.nonzero(keep)                                          # row-major: centre order, then slot order
    v = idx[c, p]
    k = np.where(v < lim, v, idx[c, 0])
    info = ((c << 16) | k).astype(np.uint32)
    dxyz = np.zeros((len(c), 4), np.float32)
    dxyz[:, :3] = xyz[k].astype(np.float32) - new_xyz[c].astype(np.float32)
    out = CloudRows((info, dxyz, cnt))
    if mutant == "pad_with_last_row":
        out.pad = (info[-1], dxyz[-1].copy())
    else:
        k0 = idx[m - 1, 0]
        pad = np.zeros(4, np.float32)
        pad[:3] = xyz[k0].astype(np.float32) - new_xyz[m - 1].astype(np.float32)
        out.pad = (np.uint32(((m - 1) << 16) | k0), pad)
    return out


def row_list(idx, xyz, new_xyz, limit=None, rep=None, crep=None, _mutant=None):
    """idx (b,m,ns), xyz (b,n,3), new_xyz (b,m,3), limit (b), rep (b,n), crep (b,m) -> per cloud a CloudRows"""
    assert _mutant is None or _mutant in MUTANTS
    return [_cloud_rows(idx[i], xyz[i], new_xyz[i], None if limit is None else limit[i], None if rep is None else rep[i],
                        None if crep is None else crep[i], _mutant) for i in range(idx.shape[0])]


def tiles_of(cloud_rows):
    """the padded form of one cloud: (rowinfo u32[tiles, 64], rowdxyz f32[tiles, 64, 4])"""
    info, dxyz, _ = cloud_rows
    rows = len(info)
    tiles = (rows + ROWS - 1) // ROWS
    pi = np.full(tiles * ROWS, cloud_rows.pad[0], np.uint32)
    pd = np.tile(cloud_rows.pad[1], (tiles * ROWS, 1)).astype(np.float32)
    pi[:rows], pd[:rows] = info, dxyz
    return pi.reshape(tiles, ROWS), pd.reshape(tiles, ROWS, 4)


def packed_list(clouds):
    """the list of `clouds` (CloudRows of consecutive clouds) in cloud order: (rowinfo u32[T*64], rowdxyz f32[T*64, 4], tilecloud
    i32[T], hdr (tiles, rows)) -- what a deterministic producer writes; one that draws tiles from a counter permutes the clouds"""
    t = [tiles_of(c) for c in clouds]
    info = np.concatenate([a.reshape(-1) for a, _ in t])
    dxyz = np.concatenate([d.reshape(-1, 4) for _, d in t])
    tilecloud = np.repeat(np.arange(len(clouds), dtype=np.int32), [a.shape[0] for a, _ in t])
    return info, dxyz, tilecloud, (len(tilecloud), sum(len(c[0]) for c in clouds))


# ------------------------------------------------------------------------------------------------------------------ generators
def ball_like(rng, b, m, n, ns, mean_cnt):
    """index rows shaped like a ball query's output: cnt distinct increasing indices, then copies of the first"""
    idx = np.empty((b, m, ns), np.int32)
    cnt = np.clip(rng.geometric(1.0 / mean_cnt, (b, m)), 1, ns)
    cnt[0, 0], cnt[-1, -1] = ns, 1
    if m > 2:
        cnt[0, 1] = 1
    for i in range(b):
        for c in range(m):
            k = np.sort(rng.choice(n, cnt[i, c], replace=False))
            idx[i, c, :cnt[i, c]] = k
            idx[i, c, cnt[i, c]:] = k[0]
    return idx, cnt


Case = collections.namedtuple("Case", ["idx", "xyz", "new_xyz", "limit", "rep", "crep", "planted"])
FORMS = ("plain", "limit", "rep", "crep", "rep+crep", "limit+crep", "limit+rep", "arbitrary")
_MEANS = (9.0, 1.5, 3.0, 30.0, 2.0, 14.0)          # very different row totals among the clouds of one list


def _fill_to_multiple(cnt, cands, ns, have):
    """raise counts of the centres `cands` until have + their sum is a multiple of 64"""
    need = (-(have + int(cnt[cands].sum()))) % ROWS
    for c in cands:
        add = min(need, ns - int(cnt[c]))
        cnt[c] += add
        need -= add
    assert need == 0, "not enough centres to reach a multiple of 64"


def make_case(form, b, m, n, ns, seed, ball_only=False):
    """Seeded input of one form ("plain", "limit", "rep", "crep" joined by "+", or "arbitrary": rows without any structure), b >= 3.
    The contracts: limit -- the points k >= lim are exact copies of k % lim, rows sorted so that a copy's original comes first;
    rep -- an idempotent map with rep[k] <= k, copies share coordinates, a copy's representative sits earlier in the same row;
    crep -- the same over the centres, a copy centre has its representative's coordinates and its index row.
    The edge cases the kernels' branches need are planted and ASSERTED (Case.planted: name -> True).  ball_only: without the one row
    that no ball query returns (`limit`: a slot >= lim inside the kept prefix) -- for comparisons that hold for ball-shaped rows only."""
    assert form in FORMS and b >= (3 if form in ("plain", "rep", "arbitrary") else 4) and ns >= 4 and n >= 4 * ns
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2, 2, (b, n, 3)).astype(np.float32)
    new_xyz = rng.uniform(-2, 2, (b, m, 3)).astype(np.float32)
    if form == "arbitrary":
        idx = rng.integers(0, 6, (b, m, ns)).astype(np.int32)                # heavy repetition, no structure
        idx[0, 0] = 5
        idx[1, 1] = np.arange(ns)
        idx[2, 2, min(10, ns - 1):] = idx[2, 2, 0]
        cnt = [c[2] for c in row_list(idx, xyz, new_xyz)]
        planted = {"full_row": bool(cnt[1][1] == ns), "cnt_one": bool(cnt[0][0] == 1),
                   "padding_is_not_the_last_row": any(c[m - 1] >= 2 and c.sum() % ROWS for c in cnt)}
        assert all(planted.values()), planted
        return Case(idx, xyz, new_xyz, None, None, None, planted)
    parts = form.split("+")
    has_lim, has_rep, has_crep = "limit" in parts, "rep" in parts, "crep" in parts
    arange_m = np.arange(m)
    nchunk = (m + CHUNK - 1) // CHUNK

    # ---- the points: which are copies of which
    limit = rep = crep = None
    lim = np.full(b, n, np.int64)
    if has_lim:
        lim = rng.integers(max(ns + 8, n // 4), n // 2 + 1, b)                # every original has at least one copy
        limit = lim.astype(np.int32)
        limit[1], limit[2] = 1, 0                                            # clouds whose points are all one point
        lim[1] = lim[2] = 1
        for i in range(b):
            xyz[i] = xyz[i, np.arange(n) % lim[i]]
    if has_rep:
        rep = np.empty((b, n), np.int32)
        for i in range(b):
            own = rng.random(lim[i]) < 0.75
            own[:16] = True
            owners = np.nonzero(own)[0]
            base = np.arange(lim[i])
            for k in np.nonzero(~own)[0]:
                base[k] = owners[rng.integers(0, np.searchsorted(owners, k))]
            rep[i] = base[np.arange(n) % lim[i]]
            xyz[i] = xyz[i, rep[i]]
    if has_crep:
        crep = np.tile(arange_m.astype(np.int32), (b, 1))
        for i in range(b):
            own = rng.random(m) < 0.7
            own[:3] = True
            if i == 0:
                own[m - 1] = False                                           # a last centre that is a copy
            if i == 1 and nchunk >= 3:
                own[CHUNK * (nchunk // 2):CHUNK * (nchunk // 2 + 1)] = False  # a workgroup of the write kernel without rows: in the middle
                own[CHUNK * (nchunk - 1):] = False                           # ... and as the (possibly short) last chunk
            if i == 2:
                own[5:] = False                                              # a cloud of a handful of rows
            if i == 3:
                own[m - 1] = True                                            # a last centre with rows of its own
            owners = np.nonzero(own)[0]
            for c in np.nonzero(~own)[0]:
                crep[i, c] = owners[rng.integers(0, np.searchsorted(owners, c))]
    own_c = np.ones((b, m), bool) if crep is None else crep == arange_m[None]

    # ---- the counts: distinct rows every centre is to list
    avail = np.array([int(((rep[i, :lim[i]] == np.arange(lim[i])).sum()) if has_rep else lim[i]) for i in range(b)])
    mean = np.minimum(np.array([_MEANS[i % len(_MEANS)] for i in range(b)]), ns / 2.0)
    cnt = np.clip(rng.geometric(1.0 / mean[:, None], (b, m)), 1, ns)
    cnt = np.minimum(cnt, avail[:, None])
    cnt[0, 0], cnt[0, 1] = ns, 1
    odd = has_lim and not ball_only                # a non-ball row: a slot >= lim inside the kept prefix (cloud 0, centre 2)
    if odd:
        cnt[0, 2] = 3 if has_rep else 4
    if has_crep:
        cnt[2, :5] = np.minimum(cnt[2, :5], 8)
    elif m < ROWS:
        cnt[2] = np.minimum(cnt[2], 1 + (arange_m % 7 == 0))                 # a cloud of fewer than 64 rows in all
    j = 3 if has_lim or has_crep else 2                                      # a padded cloud whose last row is NOT its padding row
    cnt[j, m - 1] = max(cnt[j, m - 1], 2)
    # cloud 0: the rows of chunk 0 a multiple of 64 (a tile that starts exactly on a chunk boundary), and the cloud's total as well
    fixed = 3
    if m > CHUNK:
        cands = [c for c in range(fixed, CHUNK) if own_c[0, c]]
        _fill_to_multiple(cnt[0], cands, ns, int(cnt[0, :fixed].sum()))
        cands = [c for c in range(CHUNK, m) if own_c[0, c]]
        _fill_to_multiple(cnt[0], cands[::-1], ns, 0)
    else:
        cands = [c for c in range(fixed, m) if own_c[0, c]]
        _fill_to_multiple(cnt[0], cands, ns, int(cnt[0, :fixed].sum()))

    # ---- the index rows
    idx = np.empty((b, m, ns), np.int32)
    for i in range(b):
        L = int(lim[i])
        pts = np.nonzero(rep[i, :L] == np.arange(L))[0] if has_rep else np.arange(L)
        copies_of = None
        if has_rep:                                                          # the points that are not their own representative, by representative
            copies_of = collections.defaultdict(list)
            for k in np.nonzero(rep[i] != np.arange(n))[0]:
                if k < L or not has_lim:
                    copies_of[int(rep[i, k])].append(int(k))
        for c in range(m):
            if not own_c[i, c]:
                continue
            q = int(cnt[i, c])
            kept = np.sort(rng.choice(pts, q, replace=False))
            extra = []
            room = ns - q
            if room and has_lim:                                             # wrap-around copies k = s + j lim of listed originals
                for s in rng.permutation(kept)[:room]:
                    if s + L < n and len(extra) < min(room, 3):
                        extra.append(int(s + L * rng.integers(1, (n - 1 - s) // L + 1)))
            if room and has_rep:                                             # copies whose representative is listed
                for s in rng.permutation(kept):
                    if copies_of[int(s)] and len(extra) < min(room, 5):
                        extra.append(copies_of[int(s)][rng.integers(0, len(copies_of[int(s)]))])
            row = np.sort(np.unique(np.concatenate([kept, np.array(extra, np.int64)])))
            idx[i, c, :len(row)] = row
            idx[i, c, len(row):] = row[0]
    if odd:
        L = int(lim[0])
        a, mid, z = 1, 2, 5                                                   # own representatives: points 0 .. 15 always are
        idx[0, 2] = a
        idx[0, 2, :4] = (a, mid, L + mid, z)                                 # the copy of `mid` sits before the last kept slot
    if has_crep:
        for i in range(b):
            new_xyz[i] = new_xyz[i, crep[i]]
            idx[i] = idx[i, crep[i]]

    # ---- what was planted
    clouds = row_list(idx, xyz, new_xyz, limit, rep, crep)
    got = np.stack([c[2] for c in clouds])
    assert np.array_equal(got, np.where(own_c, cnt, 0)), "the rows do not list the planned counts"
    totals = got.sum(1)
    planted = {"full_row": bool((got == ns).any()), "cnt_one": bool((got == 1).any()),
               "total_multiple_of_64": bool((totals % ROWS == 0).any()), "total_not_multiple_of_64": bool((totals % ROWS != 0).any())}
    planted["padding_is_not_the_last_row"] = bool(((totals % ROWS != 0) & (got[:, m - 1] != 1)).any())       # (a last centre without rows still pads)
    if m < ROWS or has_crep:                                                 # (without crep a cloud lists at least m rows)
        planted["fewer_than_64_rows"] = bool((totals < ROWS).any())
    if m > CHUNK:
        before = np.cumsum(got.reshape(b, -1)[:, :CHUNK * (nchunk - 1)].reshape(b, nchunk - 1, CHUNK).sum(2), 1)   # rows before chunks 1 ..
        mine = np.stack([got[:, CHUNK * k:CHUNK * (k + 1)].sum(1) for k in range(1, nchunk)], 1)
        planted["tile_starts_on_a_chunk_boundary"] = bool(((before % ROWS == 0) & (mine > 0)).any())
        planted["tile_straddles_a_chunk_boundary"] = bool(((before % ROWS != 0) & (mine > 0)).any())
        planted["short_last_chunk_with_rows"] = bool(m % CHUNK == 0 or (got[:, CHUNK * (nchunk - 1):].sum(1) > 0).any())
    if has_crep:
        planted["last_centre_is_a_copy"] = bool((crep[:, m - 1] != m - 1).any())
        planted["last_centre_owns_rows"] = bool((crep[:, m - 1] == m - 1).any())
        assert all((crep[i, crep[i]] == crep[i]).all() and (crep[i] <= arange_m).all() for i in range(b))
        if m >= TWO_LAUNCH_M:
            empty = np.stack([got[:, CHUNK * k:CHUNK * (k + 1)].sum(1) == 0 for k in range(nchunk)], 1)
            planted["empty_chunk_in_the_middle"] = bool(empty[:, 1:nchunk - 1].any())
            planted["empty_last_chunk"] = bool(empty[:, nchunk - 1].any())
    if has_lim:
        in_prefix = (idx >= lim[:, None, None]) & (np.arange(ns)[None, None, :] < got[:, :, None])
        if odd:
            planted["slot_beyond_limit_inside_the_prefix"] = bool(in_prefix.any()) if not has_rep else bool((idx[0, 2, 2] >= lim[0]) and got[0, 2] == 3)
        else:
            assert not in_prefix.any()
        planted["limit_zero_and_one"] = bool((limit == 0).any() and (limit == 1).any())
        planted["copies_listed_after_originals"] = bool((idx >= lim[:, None, None]).sum() > b * m // 4)
    if has_rep:
        mine = np.stack([rep[i][idx[i]] for i in range(b)])
        dropped = (mine != idx) & own_c[:, :, None]
        later_kept = np.flip(np.maximum.accumulate(np.flip((mine == idx) & (idx != idx[:, :, :1]), 2), 2), 2)
        planted["copy_before_a_kept_slot"] = bool((dropped & later_kept).any())
        assert all((rep[i, rep[i]] == rep[i]).all() and (rep[i] <= np.arange(n)).all() for i in range(b))
    assert all(planted.values()), planted
    return Case(idx, xyz, new_xyz, limit, rep, crep, planted)


# ------------------------------------------------------------------------------------------------------------------ the cases
# (form, b, m, n, nsample): b in 3..6, n = 2048 (512 where `limit` models RoI clouds), nsample 30 reaches the scalar path (ns & 3) != 0.
def _cases(forms, ms, nss, every=False):
    out, k = [], 0
    for form in forms:
        for m in ms:
            for ns in (nss if every else (nss[k % len(nss)],)):
                lo = 3 if form in ("plain", "rep", "arbitrary") else 4       # (limit / crep use up clouds 0 .. 2 for their edge cases)
                out.append((form, lo if m >= 1024 else lo + k % (7 - lo), m, 512 if "limit" in form else 2048, ns))
                k += 1
    return out


ONE_WORKGROUP = _cases(FORMS, (37, 511), (64, 30, 16, 32))                                     # ball_pack_kernel: m < 512, or any rep
TWO_LAUNCH = _cases(("plain", "limit", "crep", "limit+crep"), (512, 600, 1024), (16, 30, 32, 64), every=True)
_cache = {}


def case(form, b, m, n, ns, ball_only=False):
    """make_case, made once per process and shared: (Case, its row_list).  Nobody writes into the arrays."""
    key = (form, b, m, n, ns, ball_only)
    if key not in _cache:
        c = make_case(form, b, m, n, ns, seed=1000 * m + 10 * ns + FORMS.index(form), ball_only=ball_only)
        _cache[key] = (c, row_list(c.idx, c.xyz, c.new_xyz, c.limit, c.rep, c.crep))
    return _cache[key]


def case_id(c):
    return "%s-b%d-m%d-n%d-ns%d" % c
