"""Road planes of a KITTI-format tree, estimated from the LiDAR sweeps: ``planes/%06d.txt`` for datasets that ship none (Argoverse,
nuScenes, Lyft, Waymo brought into KITTI format, or a tree rescaled by stat_norm convert).  The files are what aug_scene.road_plane, the
online GT-aug of train_input.py and kitti_eval --toground read.  The reference project has no tool for this; the estimator is this
package's own.

  estimate_planes(scenes, ...)   the estimator for a batch: device="cuda" runs csrc/road_planes.hip in one call with ONE device-to-host
                                 read; device="cpu" is the numpy restatement, hypothesis by hypothesis (the checker, not a second
                                 product path; neither path falls back to the other)
  write_plane(path, plane)       KITTI's plane format
  generate_planes(root, ...)     the tool

Command line:
  python -m 3d_adapt_auto_driving_amd.road_planes --root R [--split train] [--save_dir D] [--overwrite] [--check] [--iters 512]
         [--thresh 0.2] [--max_tilt_deg 15] [--x_range -20 20] [--z_range 0 50] [--min_inliers 100] [--default_height 1.65] [--seed 0]
         [--batch 8] [--device cuda|cpu]

Read: ``<root>/KITTI/ImageSets/<split>.txt`` and ``velodyne/``, ``calib/`` of ``<root>/KITTI/object/training`` (``testing`` for the split
``test``); no image, no label.  Written: ``planes/%06d.txt`` there, or ``<save_dir>/%06d.txt``, and ``planes_log.txt`` next to them.  A
scene whose plane file exists stops the run before anything is written unless ``--overwrite`` is given.  ``--check`` writes nothing: for
every scene that has a plane file it prints the angle between the stored and the estimated normal and the difference of the heights
under the sensor (-d / b), then the split's median and maximum of both.

The estimator (both paths; f64 on the f32 rect coordinates, one rounding per operation, sums left to right):
  1. rect coordinates: kitti_io.Calibration.lidar_to_rect, f32;
  2. candidates: the points with x_range[0] <= x <= x_range[1] and z_range[0] <= z <= z_range[1], in point order; M of them;
  3. draws: u = RandomState(seed + sample_id).random_sample((iters, 3)) per scene, before any geometry;
  4. hypothesis h: the candidates min(floor(u[h, j] M), M - 1); n = (p1 - p0) x (p2 - p0), L = sqrt(n . n), rejected unless L > 1e-6;
     n / L, flipped when n_y > 0; rejected unless -n_y >= cos(max_tilt); d = -(n . p0), rejected unless d > 0;
  5. score: the candidates with |n_x x + n_y y + n_z z + d| <= thresh; the largest score wins, among equals the smallest h;
  6. fallback (0, -1, 0, default_height) when M < 3, when no hypothesis survives or when the winner's score is below min_inliers;
  7. two refits, each over the inliers of the current plane under the same test: moments n, Sx, Sz, Sy, Sxx, Sxz, Szz, Sxy, Szy of the
     coordinates shifted by the winner's first point p0, y' = alpha x' + beta z' + gamma by Cramer's rule, (a, b, c, d) =
     (alpha, -1, beta, -alpha p0_x + p0_y - beta p0_z + gamma) / sqrt(alpha^2 + 1 + beta^2); a refit whose determinant is zero or not
     finite, or that leaves the tilt bound or d > 0, is discarded and the plane before it kept;
  8. inliers and rms (of the signed distances of the inliers) are the final plane's.
The device path equals the cpu path in every integer and flag; the plane and rms differ by the order of the moment sums only.
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import math
import os

import numpy as np

from . import _lib, kitti_io
from .scene_batch import MAX_IO_WORKERS, as_calib, check_device, pack_scenes, upload_arrays as _upload

FALLBACK_REASONS = (None, "fewer than 3 candidates", "no hypothesis survived the tilt and height tests", "best score below min_inliers")
INFO_FIELDS = ("candidates", "best_hypothesis", "ransac_inliers", "inliers", "rms", "fallback")
LOG_NAME = "planes_log.txt"


class _Params:
    def __init__(self, iters, thresh, max_tilt_deg, x_range, z_range, min_inliers, default_height):
        self.iters, self.thresh, self.min_inliers, self.default_height = int(iters), float(thresh), int(min_inliers), float(default_height)
        self.cos_tilt = math.cos(math.radians(float(max_tilt_deg)))
        (self.x0, self.x1), (self.z0, self.z1) = (float(v) for v in x_range), (float(v) for v in z_range)
        if self.iters < 1:
            raise ValueError("road_planes: iters must be at least 1")


def draws_of(seed, sample_id, iters):
    """The stream of one scene: it depends on no geometric result"""
    return np.random.RandomState(int(seed) + int(sample_id)).random_sample((int(iters), 3))


def _info(candidates, best, ransac, inliers, rms, code):
    return dict(zip(INFO_FIELDS, (int(candidates), int(best), int(ransac), int(inliers), float(rms), FALLBACK_REASONS[int(code)])))


# --------------------------------------------------------------------------------------------------------------------- cpu path
def _left_sum(v):
    """v[0] + v[1] + ... left to right (np.sum adds pairwise)"""
    return float(np.add.accumulate(v)[-1]) if len(v) else 0.0


def _signed(plane, X, Y, Z):
    a, b, c, d = plane
    return ((a * X + b * Y) + c * Z) + d


def _refit(plane, p0, X, Y, Z, p):
    """One refit -> the new plane, or ``plane`` where the refit is discarded"""
    keep = np.abs(_signed(plane, X, Y, Z)) <= p.thresh
    xs, ys, zs = X[keep] - p0[0], Y[keep] - p0[1], Z[keep] - p0[2]
    n = float(len(xs))
    Sx, Sz, Sy = _left_sum(xs), _left_sum(zs), _left_sum(ys)
    Sxx, Sxz, Szz, Sxy, Szy = _left_sum(xs * xs), _left_sum(xs * zs), _left_sum(zs * zs), _left_sum(xs * ys), _left_sum(zs * ys)
    m00, m01, m02 = Szz * n - Sz * Sz, Sxz * n - Sz * Sx, Sxz * Sz - Szz * Sx
    det = (Sxx * m00 - Sxz * m01) + Sx * m02
    if not math.isfinite(det) or det == 0.0:
        return plane
    da = (Sxy * m00 - Sxz * (Szy * n - Sz * Sy)) + Sx * (Szy * Sz - Szz * Sy)
    db = (Sxx * (Szy * n - Sz * Sy) - Sxy * m01) + Sx * (Sxz * Sy - Szy * Sx)
    dg = (Sxx * (Szz * Sy - Szy * Sz) - Sxz * (Sxz * Sy - Szy * Sx)) + Sxy * m02
    alpha, beta, gamma = da / det, db / det, dg / det
    norm = math.sqrt((alpha * alpha + 1.0) + beta * beta)
    a, b, c = alpha / norm, -1.0 / norm, beta / norm
    d = ((((-alpha) * p0[0] + p0[1]) - beta * p0[2]) + gamma) / norm
    if not (-b >= p.cos_tilt) or not (d > 0.0) or not all(math.isfinite(v) for v in (a, c, d)):
        return plane
    return (a, b, c, d)


def _plane_cpu(pts, calib, u, p, details):
    rect = np.ascontiguousarray(calib.lidar_to_rect(pts[:, 0:3]), dtype=np.float32)
    x, z = rect[:, 0].astype(np.float64), rect[:, 2].astype(np.float64)
    cand = rect[(x >= p.x0) & (x <= p.x1) & (z >= p.z0) & (z <= p.z1)]
    M = len(cand)
    X, Y, Z = (cand[:, k].astype(np.float64) for k in range(3))
    accepted, scores, hyp = np.zeros(p.iters, dtype=bool), np.zeros(p.iters, dtype=np.int64), np.zeros((p.iters, 7))
    if M >= 3:
        t = np.floor(u * float(M))
        idx = np.where(t >= 0.0, np.minimum(t, M - 1), 0.0).astype(np.int64)
        for h in range(p.iters):
            i0, i1, i2 = idx[h]
            p0 = (float(X[i0]), float(Y[i0]), float(Z[i0]))
            e1 = (float(X[i1]) - p0[0], float(Y[i1]) - p0[1], float(Z[i1]) - p0[2])
            e2 = (float(X[i2]) - p0[0], float(Y[i2]) - p0[1], float(Z[i2]) - p0[2])
            nx, ny, nz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
            L = math.sqrt((nx * nx + ny * ny) + nz * nz)
            if not L > 1e-6:
                continue
            nx, ny, nz = nx / L, ny / L, nz / L
            if ny > 0.0:
                nx, ny, nz = -nx, -ny, -nz
            d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
            if not (-ny >= p.cos_tilt) or not (d > 0.0):
                continue
            accepted[h] = True
            scores[h] = np.count_nonzero(np.abs(_signed((nx, ny, nz, d), X, Y, Z)) <= p.thresh)
            hyp[h] = (nx, ny, nz, d) + p0
    plane, best, ransac = (0.0, -1.0, 0.0, p.default_height), -1, 0
    if M < 3:
        code = 1
    elif not accepted.any():
        code = 2
    else:
        first = int(np.argmax(np.where(accepted, scores, -1)))                  # the first of the largest
        ransac = int(scores[first])
        code = 3 if ransac < p.min_inliers else 0
        if code == 0:
            best, plane = first, tuple(float(v) for v in hyp[first, 0:4])
            for _ in range(2):
                plane = _refit(plane, hyp[first, 4:7], X, Y, Z, p)
    dist = _signed(plane, X, Y, Z)
    dist = dist[np.abs(dist) <= p.thresh]
    rms = math.sqrt(_left_sum(dist * dist) / float(len(dist))) if len(dist) else 0.0
    info = _info(M, best, ransac, len(dist), rms, code)
    if details:
        info.update(candidate_points=cand.copy(), accepted=accepted, scores=scores)
    return np.asarray(plane, dtype=np.float64), info


# ------------------------------------------------------------------------------------------------------------------ device path
def _launch_device(clouds, calibs, draws, p, device):
    """Upload and every launch of a call, NO host read -> (pack, the device arrays by name; ``out`` is what the caller reads)"""
    import torch
    S = len(clouds)
    pk = pack_scenes(clouds, [0] * S, calibs)
    total = int(pk.pt_off[-1])
    if total >= 2 ** 31:
        raise ValueError("road_planes batch too large: split it")
    groups = max(1, -(-pk.max_tiles // _lib.PRCNN_RP_GROUP_TILES))
    if S * groups * p.iters >= 2 ** 31:
        raise ValueError("road_planes batch too large: split it")
    host = [np.ascontiguousarray(a) for a in (pk.pt_off.astype(np.int32), pk.tile_off.astype(np.int32), pk.velo.astype(np.float32),
                                              pk.calib.astype(np.float32), np.stack(draws).astype(np.float64))]
    buf, (a_pt, a_tile, a_velo, a_calib, a_draws) = _upload(host, device)

    def work(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=device)

    t_tile_cnt, t_cand_n = work((max(1, int(pk.tile_off[-1])),), torch.int32), work((S,), torch.int32)
    t_cand, t_hyp = work((max(1, total), 4), torch.float32), work((S, p.iters, _lib.PRCNN_RP_HYP), torch.float64)
    t_part, t_scores = work((S, groups, p.iters), torch.int32), work((S, p.iters), torch.int32)
    t_p0, t_mom = work((S, 4), torch.float64), work((S, _lib.PRCNN_RP_MOMENT_GROUPS, _lib.PRCNN_RP_MOM), torch.float64)
    t_out = work((S, _lib.PRCNN_RP_OUT), torch.float64)
    _lib.call("prcnn_road_planes", S, pk.max_tiles, p.iters, a_pt, a_tile, a_velo, a_calib, a_draws, p.x0, p.x1, p.z0, p.z1, p.thresh,
              p.cos_tilt, p.min_inliers, p.default_height, t_tile_cnt.data_ptr(), t_cand_n.data_ptr(), t_cand.data_ptr(), t_hyp.data_ptr(),
              t_part.data_ptr(), t_scores.data_ptr(), t_p0.data_ptr(), t_mom.data_ptr(), t_out.data_ptr(), C.c_void_p(_lib.current_stream(buf)))
    return pk, dict(inputs=buf, out=t_out, cand=t_cand, hyp=t_hyp, scores=t_scores)


def _planes_device(clouds, calibs, draws, p, device, details):
    pk, t = _launch_device(clouds, calibs, draws, p, device)
    out = t["out"].cpu().numpy()                                                # the ONE device-to-host read of a call
    infos = [_info(r[5], r[6], r[7], r[8], r[4], r[9]) for r in out]
    if details:                                                                 # (the tests' view of the stages: further reads)
        cand, hyp, scores = t["cand"].cpu().numpy(), t["hyp"].cpu().numpy(), t["scores"].cpu().numpy()
        for s, info in enumerate(infos):
            o = int(pk.pt_off[s])
            info.update(candidate_points=cand[o:o + info["candidates"], 0:3].copy(), accepted=hyp[s, :, 7] != 0.0,
                        scores=scores[s].astype(np.int64))
    return out[:, 0:4].copy(), infos


def estimate_planes(scenes, device="cuda", iters=512, thresh=0.2, max_tilt_deg=15.0, x_range=(-20, 20), z_range=(0, 50), min_inliers=100,
                    default_height=1.65, seed=0, ids=None, u=None, details=False):
    """scenes: iterable of (points (n, 4) f32 in the LiDAR frame, calibration (kitti_io.Calibration, a calib file path or its dict)).
    ``ids``: the scenes' sample ids (the draws of a scene are RandomState(seed + sample_id)'s; by default its position in ``scenes``);
    ``u``: per scene the draws themselves, (iters, 3) f64 in [0, 1), in place of the seeded ones.
    -> planes (S, 4) f64 [a, b, c, d]: unit normal, b < 0 (up, in the rect frame), d > 0;
       info: per scene a dict of candidates, best_hypothesis (-1: fallback), ransac_inliers, inliers, rms, fallback (the reason, or None);
       with ``details`` also candidate_points (M, 3) f32 in point order, accepted (iters,) bool and scores (iters,) per hypothesis."""
    p = _Params(iters, thresh, max_tilt_deg, x_range, z_range, min_inliers, default_height)
    scenes = [(np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 4)), as_calib(calib)) for pts, calib in scenes]
    S = len(scenes)
    ids = list(range(S)) if ids is None else [int(i) for i in ids]
    if len(ids) != S or (u is not None and len(u) != S):
        raise ValueError("road_planes: ids and u name every scene")
    draws = [draws_of(seed, i, p.iters) for i in ids] if u is None else [np.asarray(v, dtype=np.float64).reshape(p.iters, 3) for v in u]
    if S == 0:
        return np.zeros((0, 4), dtype=np.float64), []
    if str(device) == "cpu":
        with np.errstate(all="ignore"):
            got = [_plane_cpu(pts, calib, d, p, details) for (pts, calib), d in zip(scenes, draws)]
        return np.stack([g[0] for g in got]), [g[1] for g in got]
    check_device(device)
    return _planes_device([pts for pts, _ in scenes], [c for _, c in scenes], draws, p, device, details)


# ------------------------------------------------------------------------------------------------------------------------ tool
def write_plane(path, plane):
    """KITTI's plane file: ``# Plane``, ``Width 4``, ``Height 1`` and ``a b c d`` printed %e"""
    with open(path, "w") as f:
        f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%e" % float(v) for v in plane))


def plane_difference(stored, estimated):
    """-> (angle between the normals in degrees, difference of the heights under the sensor -d / b in metres)"""
    ns, ne = np.asarray(stored[0:3], dtype=np.float64), np.asarray(estimated[0:3], dtype=np.float64)
    angle = math.degrees(math.atan2(float(np.linalg.norm(np.cross(ns, ne))), float(np.dot(ns, ne))))
    return angle, abs(-stored[3] / stored[1] - (-estimated[3] / estimated[1]))


def _info_line(sample_id, plane, info):
    return "%06d candidates=%d best_hypothesis=%d ransac_inliers=%d inliers=%d rms=%.6f plane=%s fallback=%s" % (
        sample_id, info["candidates"], info["best_hypothesis"], info["ransac_inliers"], info["inliers"], info["rms"],
        ",".join("%e" % v for v in plane), info["fallback"])


def generate_planes(root, split="train", save_dir=None, overwrite=False, check=False, device="cuda", batch=8, workers=8, log=print, **estimator):
    """The tool on ``root/KITTI/object/training`` (``testing`` for the split ``test``) over ``KITTI/ImageSets/<split>.txt``.
    ``estimator``: estimate_planes' keywords (iters, thresh, max_tilt_deg, x_range, z_range, min_inliers, default_height, seed).
    -> per scene (sample id, plane (4,) f64, info); with ``check`` per scene that has a plane file (sample id, angle in degrees, height
    difference in metres), nothing written."""
    from .gt_database import sample_id_list
    if str(device) != "cpu":
        check_device(device)
    ids = [int(x) for x in sample_id_list(root, split)]
    base = os.path.join(root, "KITTI", "object", "testing" if split == "test" else "training")
    plane_dir = save_dir if save_dir is not None else os.path.join(base, "planes")

    def plane_file(sample_id):
        return os.path.join(plane_dir, "%06d.txt" % sample_id)

    if check:
        ids = [i for i in ids if os.path.exists(plane_file(i))]
    elif not overwrite:
        for i in ids:
            if os.path.exists(plane_file(i)):
                raise FileExistsError("road_planes: %s exists (give --overwrite to replace the plane files)" % plane_file(i))

    def load(sample_id):
        pts = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
        return pts, kitti_io.Calibration(os.path.join(base, "calib", "%06d.txt" % sample_id))

    batch = max(1, int(batch))
    groups = [ids[k:k + batch] for k in range(0, len(ids), batch)]
    results = []
    with cf.ThreadPoolExecutor(max_workers=max(1, min(MAX_IO_WORKERS, int(workers)))) as pool:
        pending = [pool.submit(load, i) for i in groups[0]] if groups else []
        for gi, group in enumerate(groups):
            loaded = [f.result() for f in pending]
            pending = [pool.submit(load, i) for i in groups[gi + 1]] if gi + 1 < len(groups) else []
            planes, infos = estimate_planes(loaded, device=device, ids=group, **estimator)
            results += [(i, planes[k], infos[k]) for k, i in enumerate(group)]
    if check:
        from .aug_scene import road_plane                                       # the stored plane as its consumers read it
        figures = [(i,) + plane_difference(road_plane(plane_file(i)), plane) for i, plane, _ in results]
        for i, angle, height in figures:
            log("%06d angle %.6f deg height %.6f m" % (i, angle, height))
        if figures:
            ang, hgt = np.array([f[1] for f in figures]), np.array([f[2] for f in figures])
            log("%s: %d scenes with a plane file; angle median %.6f max %.6f deg; height median %.6f max %.6f m" % (
                split, len(figures), np.median(ang), ang.max(), np.median(hgt), hgt.max()))
        else:
            log("%s: no scene with a plane file under %s" % (split, plane_dir))
        return figures
    os.makedirs(plane_dir, exist_ok=True)
    fallbacks = [i for i, _, info in results if info["fallback"] is not None]
    with open(os.path.join(plane_dir, LOG_NAME), "w") as f:
        for i, plane, info in results:
            write_plane(plane_file(i), plane)
            print(_info_line(i, plane, info), file=f)
        summary = "%s: %d scenes, %d on the fallback plane%s" % (split, len(results), len(fallbacks),
                                                                 (": " + " ".join("%06d" % i for i in fallbacks)) if fallbacks else "")
        print(summary, file=f)
    log(summary)
    log("Save plane files to %s" % plane_dir)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.road_planes", description=__doc__.split("\n")[0])
    ap.add_argument("--root", type=str, default="../data/")
    ap.add_argument("--split", type=str, default="train")
    ap.add_argument("--save_dir", type=str, default=None)
    ap.add_argument("--overwrite", action="store_true", default=False)
    ap.add_argument("--check", action="store_true", default=False)
    ap.add_argument("--iters", type=int, default=512)
    ap.add_argument("--thresh", type=float, default=0.2)
    ap.add_argument("--max_tilt_deg", type=float, default=15.0)
    ap.add_argument("--x_range", type=float, nargs=2, default=(-20.0, 20.0))
    ap.add_argument("--z_range", type=float, nargs=2, default=(0.0, 50.0))
    ap.add_argument("--min_inliers", type=int, default=100)
    ap.add_argument("--default_height", type=float, default=1.65)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device", type=str, default="cuda")
    a = ap.parse_args(argv)
    generate_planes(a.root, a.split, a.save_dir, a.overwrite, a.check, a.device, a.batch, iters=a.iters, thresh=a.thresh,
                    max_tilt_deg=a.max_tilt_deg, x_range=tuple(a.x_range), z_range=tuple(a.z_range), min_inliers=a.min_inliers,
                    default_height=a.default_height, seed=a.seed)


if __name__ == "__main__":
    main()
