"""Random object scaling ("ROS") of a training batch: every labelled object's points and its box are rescaled by a factor of the
object's own, about the bottom centre of its box.  The online, statistics-free sibling of stat_norm; nothing in the reference does it,
so the definition is this module's numpy path and csrc/object_scale.hip equals it in every bit.

  scale_objects(pts, gt, counts, factors, trig=None, device="cpu", extra=None) -> pts', gt', hits

  pts      (B, N, 3) f32 rect points, numpy or torch
  gt       (B, G, 7) f32 [x, y, z, h, w, l, ry] packed with counts (B,) i32 as rpn_eval.pack_gt packs them
  trig     (B, G, 2) f32 numpy's cos / sin of the f32 ry (pack_gt's third result; computed the same way when None)
  factors  (B, G) f64
  hits     (B, G) u32: the points whose owner is box k
  extra    device path only: a second (B, N, C) f32 tensor, C = 3 | 4, whose columns 0..2 receive the same written values (the
           stage's pts_input; column 3, the intensity, is never touched)

``device="cpu"`` is the numpy definition (the checker) and returns numpy arrays.  ``device="cuda"`` runs the kernel IN PLACE on device
tensors (a host array is uploaded first) and returns device tensors and a numpy gt'.  "cuda" without a usable GPU raises
ScaleDeviceError; nothing falls back.

The definition.  All arithmetic is f64 on values widened from f32, the operations exactly as written, no contraction (the library is
built with -ffp-contract=off); no transcendental function runs on the device.
  1. Box k < counts[s] of scene s: X, Y, Z, h, w, l its f32 fields as f64, c, sn its trig as f64.  Boxes past the count are never visited.
  2. Point p: dx = px - X, dz = pz - Z, v = Y - py, a = dx*c - dz*sn, b = dx*sn + dz*c (a along the length, b along the width, v the
     height above the bottom face: KITTI's camera frame, y down, (X, Y, Z) the bottom centre).  Inside k iff
     |a| <= l*0.5 && |b| <= w*0.5 && 0 <= v && v <= h: faces are inclusive, a NaN coordinate is inside nothing.
  3. The owner of p is the lowest k that contains it, decided on the input boxes and input coordinates only; hits[s, k] counts the
     owned points, whatever the factor.
  4. r = factors[s, owner].  r == 1.0 keeps the point's bits.  Otherwise a' = a*r, b' = b*r, v' = v*r and
     px' = f32(X + (a'*c + b'*sn)), py' = f32(Y - v'), pz' = f32(Z + (b'*c - a'*sn)): the object is scaled about its bottom centre and
     stays on the road.
  5. gt'[s, k, 3:6] = f32(f64(gt[s, k, 3:6]) * r) for k below the count and r != 1.0; everything else of gt' is gt's bits (tiny host
     work, numpy on both paths).
What it deliberately does not do: points of the background or of a neighbour that a GROWN box newly encloses are left where they are,
and the gap a SHRUNK object leaves is not filled.
"""
import ctypes as C

import numpy as np

from .scene_batch import check_device


class ScaleDeviceError(RuntimeError):
    """device='cuda' was asked for and no usable device exists (nothing falls back to the numpy path)"""


def _host(a, dtype):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dtype)


def _arguments(gt, counts, factors, trig):
    gt = np.ascontiguousarray(_host(gt, np.float32))
    if gt.ndim != 3 or gt.shape[2] != 7:
        raise ValueError("scale_objects: gt must be (B, G, 7)")
    B, G = gt.shape[0], gt.shape[1]
    counts = _host(counts, np.int32).reshape(-1)
    factors = np.ascontiguousarray(_host(factors, np.float64))
    if counts.shape[0] != B or (counts > G).any() or (counts < 0).any():
        raise ValueError("scale_objects: counts must be (B,) with 0 <= count <= G")
    if factors.shape != (B, G):
        raise ValueError("scale_objects: factors must be (B, G)")
    if trig is None:
        ry = gt[:, :, 6]
        trig = np.stack([np.cos(ry), np.sin(ry)], axis=2).astype(np.float32)
    trig = np.ascontiguousarray(_host(trig, np.float32))
    if trig.shape != (B, G, 2):
        raise ValueError("scale_objects: trig must be (B, G, 2)")
    return gt, counts, factors, trig


def scale_boxes(gt, counts, factors):
    """step 5: gt' (a copy) with h, w, l of the counted boxes whose factor is not 1.0 scaled"""
    out = gt.copy()
    live = (np.arange(gt.shape[1])[None, :] < counts[:, None]) & (factors != 1.0)
    out[:, :, 3:6] = np.where(live[:, :, None], (gt[:, :, 3:6].astype(np.float64) * factors[:, :, None]).astype(np.float32), gt[:, :, 3:6])
    return out


def _scale_scene(P, boxes, trig, factors, hits):
    """steps 1-4 for one scene: P (N, 3) f32 is written in place, hits (G,) u32 is filled"""
    px, py, pz = (P[:, j].astype(np.float64) for j in range(3))
    owner = np.full(P.shape[0], -1, dtype=np.int64)
    oa, ob, ov = (np.zeros(P.shape[0], dtype=np.float64) for _ in range(3))
    for k in range(boxes.shape[0]):
        X, Y, Z, h, w, l = (np.float64(boxes[k, j]) for j in range(6))
        c, sn = np.float64(trig[k, 0]), np.float64(trig[k, 1])
        dx, dz, v = px - X, pz - Z, Y - py
        a, b = dx * c - dz * sn, dx * sn + dz * c
        with np.errstate(invalid="ignore"):
            new = (np.abs(a) <= l * 0.5) & (np.abs(b) <= w * 0.5) & (0.0 <= v) & (v <= h) & (owner < 0)
        owner[new] = k
        oa[new], ob[new], ov[new] = a[new], b[new], v[new]
        hits[k] = int(new.sum())
    for k in range(boxes.shape[0]):
        r = np.float64(factors[k])
        m = owner == k
        if r == 1.0 or not m.any():
            continue
        X, Y, Z = (np.float64(boxes[k, j]) for j in range(3))
        c, sn = np.float64(trig[k, 0]), np.float64(trig[k, 1])
        a2, b2, v2 = oa[m] * r, ob[m] * r, ov[m] * r
        P[m, 0] = (X + (a2 * c + b2 * sn)).astype(np.float32)
        P[m, 1] = (Y - v2).astype(np.float32)
        P[m, 2] = (Z + (b2 * c - a2 * sn)).astype(np.float32)


def scale_objects(pts, gt, counts, factors, trig=None, device="cpu", extra=None):
    """See the module docstring.  -> (pts', gt', hits)"""
    check_device(device)
    gt, counts, factors, trig = _arguments(gt, counts, factors, trig)
    gt2 = scale_boxes(gt, counts, factors)
    if str(device) != "cpu":
        t_pts, t_hits = _scale_device(pts, gt, counts, factors, trig, str(device), extra)
        return t_pts, gt2, t_hits
    if extra is not None:
        raise ValueError("scale_objects: extra belongs to the device path")
    P = np.array(_host(pts, np.float32), dtype=np.float32, order="C")       # a copy: the numpy path leaves its input alone
    if P.ndim != 3 or P.shape[2] != 3 or P.shape[0] != gt.shape[0]:
        raise ValueError("scale_objects: pts must be (B, N, 3)")
    hits = np.zeros(gt.shape[:2], dtype=np.uint32)
    for s in range(P.shape[0]):
        g = int(counts[s])
        with np.errstate(over="ignore"):
            _scale_scene(P[s], gt[s, :g], trig[s, :g], factors[s, :g], hits[s, :g])
    return P, gt2, hits


def _scale_device(pts, gt, counts, factors, trig, device, extra):
    """-> (pts, hits) device tensors; pts (and extra) written in place"""
    import torch
    if not torch.cuda.is_available():
        raise ScaleDeviceError("device %r asked for and no usable GPU: scale_objects does not fall back (device='cpu' is the numpy "
                               "definition)" % device)
    from . import _lib
    if not torch.is_tensor(pts):
        pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32))
    pts = pts.to(device)
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] != 3 or not pts.is_contiguous() or pts.shape[0] != gt.shape[0]:
        raise ValueError("scale_objects: pts must be a contiguous (B, N, 3) f32 tensor")
    B, N, G = int(pts.shape[0]), int(pts.shape[1]), int(gt.shape[1])
    ec = 0
    if extra is not None:
        if (not torch.is_tensor(extra) or extra.device != pts.device or extra.dtype != torch.float32 or extra.dim() != 3
                or tuple(extra.shape[:2]) != (B, N) or extra.shape[2] not in (3, 4) or not extra.is_contiguous()):
            raise ValueError("scale_objects: extra must be a contiguous (B, N, 3 | 4) f32 tensor on pts' device")
        ec = int(extra.shape[2])
    hits = torch.zeros((B, G), dtype=torch.int32, device=pts.device)        # zeroed as i32, handed out as the u32 the kernel counts in
    if B and N and G:
        up = lambda a: torch.from_numpy(a).to(pts.device, non_blocking=True)
        t_gt, t_cnt, t_trig, t_fac = up(gt), up(np.ascontiguousarray(counts)), up(trig), up(factors)
        _lib.call("prcnn_object_scale", B, N, G, pts.data_ptr(), _lib.ptr(extra), ec, t_gt.data_ptr(), t_cnt.data_ptr(), t_trig.data_ptr(),
                  t_fac.data_ptr(), hits.data_ptr(), C.c_void_p(_lib.current_stream(pts)))
    return pts, hits.view(torch.uint32)
