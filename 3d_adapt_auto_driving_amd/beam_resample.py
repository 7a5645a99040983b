"""LiDAR beam resampling of a KITTI-format tree: the beam (ring) of every point recovered from its elevation, and a copy of the tree that
keeps the rows of some beams only -- a 64-beam tree thinned to 32 or 16 beams, so that "train on A, test on B" holds the beam count fixed.
KITTI ``.bin`` rows carry no ring index.  The reference project has no tool for this; the definition is this package's own (DESIGN.md
section 38).

  edge_table(fov, bins)              the bin edges, tangents of elevations uniform in angle: made once on the host, read by both paths
  label_beams(clouds, beams, ...)    per scene the beam of every point (int32, -1 unassigned) and the clusters: centres, counts, iterations
  resample_scenes(clouds, beams, ..) the kept rows of every scene and a report
  convert_tree(src, dst, beams, ..)  the tool

device="cuda" runs csrc/beam_resample.hip (prcnn_beam_hist, prcnn_beam_lloyd, prcnn_beam_select) over the ragged batch with ONE
device-to-host read per call; device="cpu" is the numpy definition, which the device path equals in every bit.  Neither falls back to the
other: "cuda" without a usable GPU raises ResampleDeviceError.

Command line:
  python -m 3d_adapt_auto_driving_amd.beam_resample SRC DST --beams K (--stride S [--phase P] | --keep_beams I [I ...])
         [--fov LO HI] [--bins N] [--origin X Y Z] [--unassigned keep|drop] [--split S | --ids I ...] [--batch 8]
         [--overwrite] [--check] [--device cuda|cpu]

SRC and DST have the layout ``stat_norm convert`` reads and writes (the tool stands beside it in the data chain, before ``multi_data``).
Written: ``DST/training/velodyne/<id>.bin`` = the kept rows, all four floats bit for bit and in their order; every other directory of
``SRC/training`` as a link with an absolute target (as multi_data links: one that is there stays); the split files; ``DST/beam_log.txt``.
An existing ``.bin`` stops the run before anything is written unless ``--overwrite`` is given; ``--check`` writes nothing and prints the
log.  Scenes: ``--ids``, or ``SRC/<split>.txt``, by default ``trainval``.  Labels are not edited: an object left with no point stays labelled.

The definition (both paths; nothing transcendental touches a point, every sum is an integer sum):
  1. (x, y, z) = the f32 coordinates as f64 minus ``origin``; rho2 = x x + y y (products and sum rounded one by one); t = z / sqrt(rho2);
     unassigned: a non-finite coordinate, rho2 == 0;
  2. E[i] = tan(deg2rad(LO + i (HI - LO) / bins)), i = 0 .. bins, strictly increasing; a point's bin is the largest i with E[i] <= t;
     unassigned: t < E[0], t >= E[bins];
  3. a u32 histogram over the bins per scene;
  4. 1-D Lloyd on the histogram with K = ``beams`` clusters: centres lo + k (hi - lo) / (K - 1) over the lowest / highest occupied bin (lo
     for K = 1); an occupied bin goes to the nearest centre, the lower of equals; a centre becomes (sum count i) / (sum count) -- int64
     sums, one f64 division --, an empty cluster keeps its own; until no bin changes cluster, at most 64 updates;
  5. a point's beam is its bin's cluster INDEX k (0 the lowest elevation; not the rank among the non-empty clusters); the row is kept if
     k % stride == phase, or k in keep_beams; an unassigned row by ``unassigned``.
K counts the beam positions from the lowest to the highest beam that returns, both included: the centres start spread over the occupied
bins, so a sensor whose upper beams see only sky is given the count of the beams below them.  A beam that is missing between two others
leaves its cluster empty and shifts nothing.  The log's summary names every scene in which a cluster stayed empty and warns: either a
laser is dead, or K is above that count and the pattern is shifted.
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import glob
import os
import shutil

import numpy as np

from . import _lib
from .scene_batch import MAX_IO_WORKERS, check_device, pack_scenes, upload_arrays

MAX_BINS, MAX_BEAMS, MAX_ITERS = _lib.PRCNN_BEAM_MAX_BINS, _lib.PRCNN_BEAM_MAX_K, _lib.PRCNN_BEAM_MAX_ITERS
HIT_CAP, UNSORTED = _lib.PRCNN_BEAM_HIT_CAP, _lib.PRCNN_BEAM_UNSORTED
LOG_NAME = "beam_log.txt"
DEFAULT_FOV, DEFAULT_BINS = (-30.0, 10.0), 2048


class ResampleDeviceError(RuntimeError):
    """device='cuda' was asked for and no usable device exists (nothing falls back to the cpu path)"""


def _require_device(device):
    check_device(device)
    if str(device) != "cpu":
        import torch
        if not torch.cuda.is_available():
            raise ResampleDeviceError("device %r asked for and no usable GPU: beam_resample does not fall back (use --device cpu for the "
                                      "numpy definition)" % str(device))


# ------------------------------------------------------------------------------------------------------------------- parameters
def edge_table(fov=DEFAULT_FOV, bins=DEFAULT_BINS):
    """-> E (bins + 1,) f64, E[i] = tan(deg2rad(LO + i (HI - LO) / bins)): the one table of both paths.  ValueError unless it is finite and
    strictly increasing (LO < HI inside +-90 degrees) and 1 <= bins <= MAX_BINS."""
    lo, hi = (float(v) for v in fov)
    if int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError("beam_resample: bins must be an integer in 1..%d" % MAX_BINS)
    edges = np.tan(np.deg2rad(lo + (np.arange(int(bins) + 1, dtype=np.float64) * (hi - lo)) / float(int(bins))))
    if not (np.isfinite(edges).all() and (np.diff(edges) > 0.0).all()):
        raise ValueError("beam_resample: the edge table of fov (%g, %g) with %d bins is not strictly increasing" % (lo, hi, int(bins)))
    return edges


def _check_edges(edges):
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if not (2 <= len(edges) <= MAX_BINS + 1 and np.isfinite(edges).all() and (np.diff(edges) > 0.0).all()):
        raise ValueError("beam_resample: an edge table has 2..%d finite, strictly increasing entries" % (MAX_BINS + 1))
    return edges


def keep_table(beams, stride=None, phase=0, keep_beams=None):
    """-> (beams,) u8: 1 where beam k is kept: k % stride == phase, or k in keep_beams (one of the two rules)"""
    if int(beams) != beams or not 1 <= int(beams) <= MAX_BEAMS:
        raise ValueError("beam_resample: beams must be an integer in 1..%d" % MAX_BEAMS)
    k = np.arange(int(beams))
    if (stride is None) == (keep_beams is None):
        raise ValueError("beam_resample: give stride (with phase) or keep_beams, one of the two")
    if stride is not None:
        if int(stride) != stride or int(stride) < 1:
            raise ValueError("beam_resample: stride must be an integer >= 1")
        if int(phase) != phase or not 0 <= int(phase) < int(stride):
            raise ValueError("beam_resample: phase must be an integer in 0..stride - 1")
        return (k % int(stride) == int(phase)).astype(np.uint8)
    want = [int(i) for i in keep_beams]
    if any(i < 0 or i >= int(beams) for i in want):
        raise ValueError("beam_resample: keep_beams are beam indices in 0..beams - 1")
    return np.isin(k, want).astype(np.uint8)


def _origin(origin):
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("beam_resample: origin is three finite numbers")
    return o


def _unassigned(mode):
    if mode not in ("keep", "drop"):
        raise ValueError("beam_resample: unassigned is 'keep' or 'drop'")
    return int(mode == "keep")


# --------------------------------------------------------------------------------------------------------------------- cpu path
def point_bins(pts, edges, origin=(0.0, 0.0, 0.0)):
    """Steps 1 and 2 -> (n,) int32, -1 unassigned"""
    bins = len(edges) - 1
    xyz = pts[:, 0:3]
    finite = np.isfinite(xyz).all(axis=1)
    with np.errstate(all="ignore"):
        x, y, z = (xyz[:, k].astype(np.float64) - origin[k] for k in range(3))
        rho2 = x * x + y * y
        t = z / np.sqrt(rho2)
    ok = finite & (rho2 != 0.0)
    idx = np.searchsorted(edges, np.where(ok, t, 0.0), side="right") - 1          # the largest i with E[i] <= t
    ok &= (idx >= 0) & (idx < bins)
    return np.where(ok, idx, -1).astype(np.int32)


def lloyd(hist, beams):
    """Step 4 on one histogram -> (table (bins,) int32, -1 for an empty bin; centres (K,) f64; counts (K,) u32; iterations; flags)"""
    hist = np.asarray(hist).astype(np.int64)
    K, bins = int(beams), len(hist)
    table, centres, counts = np.full(bins, -1, dtype=np.int32), np.zeros(K, dtype=np.float64), np.zeros(K, dtype=np.int64)
    occ = np.flatnonzero(hist)
    if len(occ) == 0:
        return table, centres, counts.astype(np.uint32), 0, 0
    lo, hi = int(occ[0]), int(occ[-1])
    if K == 1:
        centres[0] = float(lo)
    else:
        centres[:] = float(lo) + (np.arange(K, dtype=np.int64) * (hi - lo)).astype(np.float64) / float(K - 1)
    cnt, pos = hist[occ], occ.astype(np.float64)
    assign, iters, flags = np.full(len(occ), -1, dtype=np.int64), 0, 0
    while True:
        new = np.argmin(np.abs(pos[:, None] - centres[None, :]), axis=1)         # the first of the smallest: the lower k
        if np.array_equal(new, assign):
            break
        assign = new
        num, counts = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        np.add.at(num, assign, cnt * occ)
        np.add.at(counts, assign, cnt)
        live = counts > 0
        centres[live] = num[live].astype(np.float64) / counts[live].astype(np.float64)
        iters += 1
        if iters == MAX_ITERS:
            flags |= HIT_CAP
            break
    table[occ] = assign
    if not (np.diff(centres) >= 0.0).all():
        flags |= UNSORTED
    return table, centres, counts.astype(np.uint32), iters, flags


def _scene_cpu(pts, edges, K, origin, keep, keep_un):
    pbin = point_bins(pts, edges, origin)
    hist = np.bincount(pbin[pbin >= 0], minlength=len(edges) - 1).astype(np.uint32)
    table, centres, counts, iters, flags = lloyd(hist, K)
    beam = np.where(pbin >= 0, table[np.maximum(pbin, 0)], -1).astype(np.int32)
    flag = np.where(beam >= 0, keep[np.maximum(beam, 0)] != 0, bool(keep_un))
    return dict(bins=pbin, beams=beam, hist=hist, table=table, centres=centres, counts=counts, iterations=iters, flags=flags,
                rows=np.ascontiguousarray(pts[flag]))


# ------------------------------------------------------------------------------------------------------------------ device path
def _launch_device(clouds, edges, K, origin, keep, keep_un, device):
    """Upload and every launch of a call, NO host read -> (pack, the result buffer (uint8), its sections name -> (byte offset, dtype,
    shape), the bytes a caller without ``details`` reads)"""
    import torch
    S, bins = len(clouds), len(edges) - 1
    pk = pack_scenes(clouds, [0] * S)
    total, tiles = int(pk.pt_off[-1]), int(pk.tile_off[-1])
    if total >= 2 ** 31 or S > 65535:
        raise ValueError("beam_resample batch too large: split it")
    host = [np.ascontiguousarray(a) for a in (pk.pt_off.astype(np.int32), pk.tile_off.astype(np.int32), pk.velo.astype(np.float32), edges,
                                              keep.astype(np.uint8))]
    inputs, (a_pt, a_tile, a_velo, a_edges, a_keep) = upload_arrays(host, device)
    rows = max(total, 1)
    sections, need = {}, 0
    for name, dtype, shape in (("centres", np.float64, (S, K)), ("counts", np.uint32, (S, K)), ("iterations", np.int32, (S,)),
                               ("flags", np.int32, (S,)), ("kept_n", np.int32, (S,)), ("rows", np.float32, (rows, 4)), (None, None, None),
                               ("bins", np.int32, (rows,)), ("beams", np.int32, (rows,)), ("hist", np.uint32, (S, bins)),
                               ("table", np.int32, (S, bins)), ("tile_cnt", np.int32, (max(tiles, 1),))):
        if name is None:
            lead = need                                                         # what lies in front is all a plain call reads
            continue
        sections[name] = (need, dtype, shape)
        need += (int(np.prod(shape)) * np.dtype(dtype).itemsize + 255) // 256 * 256
    out = torch.empty(need, dtype=torch.uint8, device=device)
    at = {name: out.data_ptr() + o for name, (o, _, _) in sections.items()}
    stream = C.c_void_p(_lib.current_stream(out))
    _lib.call("prcnn_beam_hist", S, pk.max_tiles, bins, a_pt, a_velo, a_edges, float(origin[0]), float(origin[1]), float(origin[2]),
              at["bins"], at["hist"], stream)
    _lib.call("prcnn_beam_lloyd", S, bins, K, at["hist"], at["table"], at["centres"], at["counts"], at["iterations"], at["flags"], stream)
    _lib.call("prcnn_beam_select", S, pk.max_tiles, bins, K, a_pt, a_tile, a_velo, at["bins"], at["table"], a_keep, int(keep_un),
              at["beams"], at["tile_cnt"], at["kept_n"], at["rows"], stream)
    return pk, dict(inputs=inputs, out=out), sections, lead


def _scenes_device(clouds, edges, K, origin, keep, keep_un, device, details):
    pk, t, sections, lead = _launch_device(clouds, edges, K, origin, keep, keep_un, device)
    end = sections["tile_cnt"][0] if details else lead
    raw = t["out"][:end].cpu().numpy()                                          # the ONE device-to-host read of a call

    def section(name):
        o, dtype, shape = sections[name]
        return raw[o:o + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)

    centres, counts, iters, flags, kept_n, rows = (section(k) for k in ("centres", "counts", "iterations", "flags", "kept_n", "rows"))
    got = []
    for s in range(len(clouds)):
        o, n = int(pk.pt_off[s]), int(pk.n[s])
        r = dict(centres=centres[s].copy(), counts=counts[s].copy(), iterations=int(iters[s]), flags=int(flags[s]),
                 rows=rows[o:o + int(kept_n[s])].copy())
        if details:
            r.update(bins=section("bins")[o:o + n].copy(), beams=section("beams")[o:o + n].copy(), hist=section("hist")[s].copy(),
                     table=section("table")[s].copy())
        got.append(r)
    return got


# -------------------------------------------------------------------------------------------------------------------------- api
def _run(clouds, beams, keep, unassigned, fov, bins, origin, edges, device, details):
    edges = edge_table(fov, bins) if edges is None else _check_edges(edges)
    origin, keep_un = _origin(origin), _unassigned(unassigned)
    _require_device(device)
    clouds = [np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1, 4)) for c in clouds]
    if not clouds:
        return []
    if str(device) == "cpu":
        got = [_scene_cpu(c, edges, int(beams), origin, keep, keep_un) for c in clouds]
    else:
        got = _scenes_device(clouds, edges, int(beams), origin, keep, keep_un, device, details)
    for s, (c, r) in enumerate(zip(clouds, got)):
        assert not r["flags"] & UNSORTED, "beam_resample: the centres of scene %d left their order" % s
        assigned = int(r["counts"].sum())
        r.update(points=len(c), kept=len(r["rows"]), unassigned=len(c) - assigned, clusters=int(np.count_nonzero(r["counts"])),
                 hit_cap=bool(r["flags"] & HIT_CAP))
    return got


def label_beams(clouds, beams, fov=DEFAULT_FOV, bins=DEFAULT_BINS, origin=(0, 0, 0), device="cuda", edges=None):
    """clouds: per scene (n, 4) f32 rows in the LiDAR frame; ``edges``: an edge table in place of edge_table(fov, bins).
    -> (ids: per scene (n,) int32, the beam of every point, -1 unassigned;
        info: per scene a dict of centres (K,) f64 in bins, counts (K,) u32 points per cluster (0: the cluster is empty), iterations,
        hit_cap, clusters (the non-empty ones), points, unassigned, and the stages bins (n,) int32, hist (bins,) u32, table (bins,) int32)"""
    got = _run(clouds, beams, keep_table(beams, stride=1), "keep", fov, bins, origin, edges, device, True)
    return [r.pop("beams") for r in got], [{k: v for k, v in r.items() if k not in ("rows", "kept", "flags")} for r in got]


def resample_scenes(clouds, beams, stride=None, phase=0, keep_beams=None, unassigned="keep", fov=DEFAULT_FOV, bins=DEFAULT_BINS,
                    origin=(0, 0, 0), device="cuda", edges=None):
    """-> (kept: per scene (m, 4) f32, the kept rows bit for bit in their order;
        report: per scene a dict of points, kept, unassigned, clusters, iterations, hit_cap, centres, counts)"""
    got = _run(clouds, beams, keep_table(beams, stride, phase, keep_beams), unassigned, fov, bins, origin, edges, device, False)
    return [r.pop("rows") for r in got], [{k: v for k, v in r.items() if k != "flags"} for r in got]


# ------------------------------------------------------------------------------------------------------------------------- tool
def _log_line(name, r):
    return "%s points=%d kept=%d unassigned=%d clusters=%d iterations=%d%s" % (name, r["points"], r["kept"], r["unassigned"], r["clusters"],
                                                                              r["iterations"], " hit_cap" if r["hit_cap"] else "")


def convert_tree(src, dst, beams, stride=None, phase=0, keep_beams=None, unassigned="keep", fov=DEFAULT_FOV, bins=DEFAULT_BINS,
                 origin=(0, 0, 0), split=None, ids=None, batch=8, overwrite=False, check=False, device="cuda", workers=8, log=print):
    """The tool (see the module's text) -> per scene (id, report).  Every argument is checked before anything is written.  Reads and writes
    run on a thread pool of ``workers`` (<= 16) while the device works on the current batch."""
    keep_table(beams, stride, phase, keep_beams)
    edges, _, _ = edge_table(fov, bins), _origin(origin), _unassigned(unassigned)
    _require_device(device)
    src = os.path.abspath(src)
    src_tr, dst_tr = os.path.join(src, "training"), os.path.join(dst, "training")
    if not os.path.isdir(os.path.join(src_tr, "velodyne")):
        raise FileNotFoundError("beam_resample: %s is not a directory" % os.path.join(src_tr, "velodyne"))
    if os.path.realpath(os.path.join(dst_tr, "velodyne")) == os.path.realpath(os.path.join(src_tr, "velodyne")):
        raise ValueError("beam_resample: DST's velodyne directory is SRC's")
    if ids is None:
        with open(os.path.join(src, "%s.txt" % (split or "trainval"))) as f:
            ids = [x.strip() for x in f.readlines() if x.strip()]
    ids = [("%06d" % i) if isinstance(i, (int, np.integer)) else str(i) for i in ids]

    def bin_file(root, i):
        return os.path.join(root, "velodyne", "%s.bin" % i)

    if not check and not overwrite:
        for i in ids:
            if os.path.lexists(bin_file(dst_tr, i)):
                raise FileExistsError("beam_resample: %s exists (give --overwrite to replace the sweeps)" % bin_file(dst_tr, i))
    if not check:
        os.makedirs(os.path.join(dst_tr, "velodyne"), exist_ok=True)
        for name in sorted(os.listdir(src_tr)):
            target, link = os.path.join(src_tr, name), os.path.join(dst_tr, name)
            if name != "velodyne" and os.path.isdir(target) and not os.path.lexists(link):      # whatever stands there stays
                os.symlink(target, link)
        for path in sorted(glob.glob(os.path.join(src, "*.txt"))):
            if os.path.basename(path) != LOG_NAME:
                shutil.copyfile(path, os.path.join(dst, os.path.basename(path)))

    def load(i):
        return np.fromfile(bin_file(src_tr, i), dtype=np.float32).reshape(-1, 4)

    def save(i, rows):
        if os.path.islink(bin_file(dst_tr, i)):                                 # replace a link, never write through it (into SRC, say)
            os.remove(bin_file(dst_tr, i))
        rows.reshape(-1).tofile(bin_file(dst_tr, i))

    batch = max(1, int(batch))
    groups = [ids[k:k + batch] for k in range(0, len(ids), batch)]
    results, writes = [], []
    with cf.ThreadPoolExecutor(max_workers=max(1, min(MAX_IO_WORKERS, int(workers)))) as pool:
        pending = [pool.submit(load, i) for i in groups[0]] if groups else []
        for gi, group in enumerate(groups):
            loaded = [f.result() for f in pending]
            pending = [pool.submit(load, i) for i in groups[gi + 1]] if gi + 1 < len(groups) else []
            kept, reports = resample_scenes(loaded, beams, stride, phase, keep_beams, unassigned, origin=origin, device=device, edges=edges)
            results += list(zip(group, reports))
            if not check:
                writes += [pool.submit(save, i, rows) for i, rows in zip(group, kept)]
        for f in writes:
            f.result()
    capped = [i for i, r in results if r["hit_cap"]]
    gaps = [i for i, r in results if 0 < r["clusters"] < int(beams)]
    lines = [_log_line(i, r) for i, r in results]
    lines.append("%d scenes, beams %d: points %d, kept %d, unassigned %d; %d scenes hit the cap of %d iterations%s; %d scenes with empty "
                 "clusters%s" % (len(results), int(beams), sum(r["points"] for _, r in results), sum(r["kept"] for _, r in results),
                                 sum(r["unassigned"] for _, r in results), len(capped), MAX_ITERS, (": " + " ".join(capped)) if capped else "",
                                 len(gaps), (": %s (WARNING: a dead laser, or --beams above the number of beam positions that return -- then "
                                             "the pattern is shifted; see the module's text)" % " ".join(gaps)) if gaps else ""))
    if check:
        for line in lines:
            log(line)
        return results
    with open(os.path.join(dst, LOG_NAME), "w") as f:
        f.write("\n".join(lines) + "\n")
    log(lines[-1])
    log("Save resampled sweeps to %s" % os.path.join(dst_tr, "velodyne"))
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.beam_resample", description=__doc__.split("\n")[0])
    ap.add_argument("src", metavar="SRC")
    ap.add_argument("dst", metavar="DST")
    ap.add_argument("--beams", type=int, required=True)
    rule = ap.add_mutually_exclusive_group(required=True)
    rule.add_argument("--stride", type=int, default=None)
    rule.add_argument("--keep_beams", type=int, nargs="+", default=None)
    ap.add_argument("--phase", type=int, default=0)
    ap.add_argument("--fov", type=float, nargs=2, default=DEFAULT_FOV, metavar=("LO", "HI"))
    ap.add_argument("--bins", type=int, default=DEFAULT_BINS)
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--unassigned", type=str, default="keep", choices=("keep", "drop"))
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--split", type=str, default=None)
    which.add_argument("--ids", type=str, nargs="+", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--overwrite", action="store_true", default=False)
    ap.add_argument("--check", action="store_true", default=False)
    ap.add_argument("--device", type=str, default="cuda")
    a = ap.parse_args(argv)
    convert_tree(a.src, a.dst, a.beams, a.stride, a.phase, a.keep_beams, a.unassigned, tuple(a.fov), a.bins, tuple(a.origin), a.split, a.ids,
                 a.batch, a.overwrite, a.check, a.device)


if __name__ == "__main__":
    main()
