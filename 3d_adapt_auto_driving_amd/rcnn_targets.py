"""The RCNN stage's training input (reference: lib/rpn/proposal_target_layer.py ProposalTargetLayer): the RPN's proposals and the ground
truth -> 64 sampled, noised RoIs per scene with their pooled, augmented, canonical point clouds and targets.  An input stage: no loss,
no optimizer, no backward pass.

  tgt = RcnnTargets(cfg, seed=None, device="cuda")
  out = tgt.forward({"roi_boxes3d": (B, M, 7), "gt_boxes3d": (B, G, 7) zero rows behind the boxes as collate_batch pads them,
                     "rpn_xyz": (B, N, 3), "rpn_features": (B, N, C), "seg_mask": (B, N), "pts_depth": (B, N),
                     "rpn_intensity": (B, N) when cfg.RCNN.USE_INTENSITY})
  out: sampled_pts (B*R, S, 3), pts_feature (B*R, S, C'), cls_label (B*R) i64, reg_valid_mask (B*R) i64, gt_of_rois (B*R, 7), gt_iou (B*R),
       roi_boxes3d (B*R, 7) with R = RCNN.ROI_PER_IMAGE, S = RCNN.NUM_POINTS.

``device="cuda"`` runs csrc/rcnn_targets.hip (and the existing RoI pooling kernel); the inputs and outputs are device tensors.
``device="cpu"`` follows the reference try by try in torch / numpy over the repository's host oracle (oracle/ext_cpu.py as the backend of
iou3d_utils and roipool3d_utils): it is the checker, not a second product path.

The random streams.  The reference draws from np.random (``permutation(fg_num)``, ``rand(ROI_PER_IMAGE)`` in the foreground-only branch,
one ``rand()`` per try) and from torch: ``randint`` on the CPU (background picks, noise level) and ``rand(..., device=box.device)`` (the
noise, the three (B, R) augmentation draws).  On a CUDA machine the latter come from the CUDA generator, which nothing here can replay;
run on the CPU -- as every fixture of this project records the reference -- they come from the one CPU generator ``randint`` uses.  THAT
is the definition this module takes: one ``np.random.RandomState(seed)`` and one CPU ``torch.Generator`` seeded alike, both consumed in
exactly the reference's order and left in exactly the state in which the reference leaves them (``generator_state()``).

The device path and the streams.  torch.rand / torch.randint consume one generator draw per element whatever the call's shape, element i
of a ``rand(P)`` pool and of a ``randint(0, 5, (P,))`` pool drawn from the same state come from the same draw, and ``RandomState.rand(P)``
equals P scalar calls (tests/test_rcnn_targets.py pins all three).  Within a scene's noise phase every numpy draw is a try draw, so the
torch position of the try at numpy position i is D x #{j < i : U[j] >= 0.2} (D = 8 draws per noised try for 'multiple', 7 for 'single'): a
prefix count over the numpy pool, taken on the host.  Per scene the host saves both states, draws pools of the largest possible size
(R x ROI_FG_AUG_TIMES numpy draws, D times as many torch draws), hands the device the per-position keep flag and noise row, reads back
how many numpy draws were used, restores the states and draws exactly that many again.  Blocking host reads per batch: one of B x 4 ints
(the three list sizes and the ground-truth count of every scene), then one int per scene.  Nothing else synchronises; ``decisions`` is
fetched from the device only when someone asks for it.
"""
import contextlib
import ctypes as C
import importlib
import threading

import numpy as np

from . import _lib

MULTIPLE_RANGES = [[0.2, 0.1, np.pi / 12, 0.7], [0.3, 0.15, np.pi / 12, 0.6], [0.5, 0.15, np.pi / 9, 0.5], [0.8, 0.15, np.pi / 6, 0.3],
                   [1.0, 0.15, np.pi / 3, 0.2]]                # pos_range, hwl_range, angle_range, mean_iou
KEEP_PROB = 0.2                                                 # a try keeps the RoI itself when rand() < 0.2
DRAWS = {"single": 7, "multiple": 8}                           # torch draws of one noised try
OUT_KEYS = ("sampled_pts", "pts_feature", "cls_label", "reg_valid_mask", "gt_of_rois", "gt_iou", "roi_boxes3d")
LIST_FG, LIST_HARD, LIST_EASY = 0, 1, 2

_backend_lock = threading.RLock()


@contextlib.contextmanager
def host_backend():
    """iou3d_utils and roipool3d_utils over the host oracle for the block (unless host stand-ins are installed already); see
    aug_scene.host_overlap_backend for the caveat about threads."""
    from . import iou3d_utils, roipool3d_utils
    with _backend_lock:
        hip = [getattr(m, "IS_HIP_EXTENSION", False) for m in (iou3d_utils.iou3d_cuda, roipool3d_utils.roipool3d_cuda)]
        if not any(hip):
            yield
            return
        try:
            ext_cpu = importlib.import_module("oracle.ext_cpu")
        except ImportError as e:
            raise RuntimeError("rcnn_targets: device='cpu' is the checker and needs the repository's oracle/ package on sys.path") from e
        saved = (iou3d_utils.iou3d_cuda, roipool3d_utils.roipool3d_cuda)
        if hip[0]:
            iou3d_utils.iou3d_cuda = ext_cpu.iou3d_cpu
        if hip[1]:
            roipool3d_utils.roipool3d_cuda = ext_cpu.roipool3d_cpu
        try:
            yield
        finally:
            iou3d_utils.iou3d_cuda, roipool3d_utils.roipool3d_cuda = saved


_AugArgs = _lib.struct("prcnn_rcnn_aug")


_TargetArgs = _lib.struct("prcnn_rcnn_target_args")


def _opt(cfg, name, default):
    return cfg[name] if name in cfg else default


class RcnnTargets:
    def __init__(self, cfg, seed=None, device="cuda"):
        import torch
        self.cfg, self.device = cfg, str(device)
        if self.device != "cpu" and not self.device.startswith("cuda"):
            raise ValueError("rcnn_targets: device must be 'cuda' or 'cpu', not %r" % (device,))
        R = cfg.RCNN
        self.method = R.REG_AUG_METHOD
        if self.method == "normal":
            raise NotImplementedError("rcnn_targets: REG_AUG_METHOD 'normal' raises in the reference as shipped (torch.rand() without a size)")
        if self.method not in DRAWS:
            raise NotImplementedError("rcnn_targets: REG_AUG_METHOD %r" % (self.method,))
        self.n_rois, self.aug_times = int(R.ROI_PER_IMAGE), int(R.ROI_FG_AUG_TIMES)
        self.fg_per_image = int(np.round(R.FG_RATIO * R.ROI_PER_IMAGE))
        self.pos_thresh = min(R.REG_FG_THRESH, R.CLS_FG_THRESH)
        if self.n_rois < 1 or self.aug_times < 0:
            raise ValueError("rcnn_targets: ROI_PER_IMAGE %d / ROI_FG_AUG_TIMES %d" % (self.n_rois, self.aug_times))
        if self.device != "cpu":
            if self.n_rois > _lib.call("prcnn_rcnn_max_rois"):
                raise ValueError("rcnn_targets: ROI_PER_IMAGE %d is above the %d the device code holds" %
                                 (self.n_rois, _lib.call("prcnn_rcnn_max_rois")))
            if self.aug_times > _lib.call("prcnn_rcnn_max_tries"):
                raise ValueError("rcnn_targets: ROI_FG_AUG_TIMES %d is above the %d the device code holds" %
                                 (self.aug_times, _lib.call("prcnn_rcnn_max_tries")))
        self.rng = np.random.RandomState(seed)
        self.tgen = torch.Generator()
        if seed is None:
            self.tgen.seed()
        else:
            self.tgen.manual_seed(int(seed))
        self._record = []                                     # what the last forward decided, per scene (see decisions)
        self.stats = {"host_reads": 0}

    # --------------------------------------------------------------------------------------------------------------- generators
    def generator_state(self):
        """(np.random state tuple, torch CPU generator state)"""
        return self.rng.get_state(), self.tgen.get_state().clone()

    def set_generator_state(self, state):
        self.rng.set_state(state[0])
        self.tgen.set_state(state[1].clone())

    @property
    def decisions(self):
        """Per scene of the last forward: sizes (fg, hard bg, easy bg list lengths), lists (the three ascending index lists), chosen
        (the R source RoIs), n_fg (how many of them are foreground), cnt / keep (R) and tried (R lists of f32 IoUs); the cpu path adds
        iou3d (M, G') and max_overlaps (M).  The device path fetches them here, not in forward."""
        out = []
        for rec in self._record:
            if "device" in rec:
                dv = rec.pop("device")
                sizes = rec["sizes"]
                lists = dv["lists"].cpu().numpy()
                rec["lists"] = [lists[q, :sizes[q]].astype(np.int64) for q in range(3)]
                rec["chosen"] = dv["src"].cpu().numpy().astype(np.int64)
                rec["cnt"] = dv["cnt"].cpu().numpy().astype(np.int64)
                rec["keep"] = dv["keep"].cpu().numpy().astype(bool)
                tried = dv["tried"].cpu().numpy()
                rec["tried"] = [[np.float32(v) for v in tried[k, :rec["cnt"][k]]] for k in range(tried.shape[0])]
                rec["max_overlaps"] = dv["max_ov"].cpu().numpy()
            out.append(rec)
        return out

    # -------------------------------------------------------------------------------------------------------------------- draws
    def _draw_bg(self, n_hard, n_easy, n_bg):
        """sample_bg_inds -> [(list, position)] from the torch stream"""
        import torch
        ri = lambda hi, k: torch.randint(low=0, high=hi, size=(k,), generator=self.tgen).long().tolist()
        if n_hard > 0 and n_easy > 0:
            k_hard = int(n_bg * self.cfg.RCNN.HARD_BG_RATIO)
            hard = ri(n_hard, k_hard)
            easy = ri(n_easy, n_bg - k_hard)
            return [(LIST_HARD, p) for p in hard] + [(LIST_EASY, p) for p in easy]
        if n_hard > 0:
            return [(LIST_HARD, p) for p in ri(n_hard, n_bg)]
        if n_easy > 0:
            return [(LIST_EASY, p) for p in ri(n_easy, n_bg)]
        raise NotImplementedError

    def _draw_picks(self, n_fg, n_hard, n_easy):
        """The sampling of proposal_target_layer.py:119-149 over the list LENGTHS -> ([(list, position)] of the R sampled RoIs,
        foreground first, and how many are foreground)"""
        R, n_bg = self.n_rois, n_hard + n_easy
        if n_fg > 0 and n_bg > 0:
            k = min(self.fg_per_image, n_fg)
            perm = self.rng.permutation(n_fg)
            fg = [(LIST_FG, int(p)) for p in perm[:k]]
            return fg + self._draw_bg(n_hard, n_easy, R - k), k
        if n_fg > 0:
            pos = np.floor(self.rng.rand(R) * n_fg).astype(np.int64)
            return [(LIST_FG, int(p)) for p in pos], R
        if n_bg > 0:
            return self._draw_bg(n_hard, n_easy, R), 0
        raise ValueError("rcnn_targets: a scene has no RoI in any of the three lists (every best IoU lies in [CLS_BG_THRESH, fg threshold))")

    def _random_aug_box3d(self, box3d):
        import torch
        g = self.tgen
        if self.method == "single":
            pos_shift = (torch.rand(3, generator=g) - 0.5)
            hwl_scale = (torch.rand(3, generator=g) - 0.5) / (0.5 / 0.15) + 1.0
            angle_rot = (torch.rand(1, generator=g) - 0.5) / (0.5 / (np.pi / 12))
        else:
            idx = int(torch.randint(low=0, high=len(MULTIPLE_RANGES), size=(1,), generator=g)[0])
            pos_shift = ((torch.rand(3, generator=g) - 0.5) / 0.5) * MULTIPLE_RANGES[idx][0]
            hwl_scale = ((torch.rand(3, generator=g) - 0.5) / 0.5) * MULTIPLE_RANGES[idx][1] + 1.0
            angle_rot = ((torch.rand(1, generator=g) - 0.5) / 0.5) * MULTIPLE_RANGES[idx][2]
        return torch.cat([box3d[0:3] + pos_shift, box3d[3:6] * hwl_scale, box3d[6:7] + angle_rot], dim=0)

    # ----------------------------------------------------------------------------------------------------------------- cpu path
    def _aug_rois_cpu(self, rois, gts, iou_src, aug_times, rec):
        """aug_roi_by_noise_torch, try by try"""
        import torch
        from . import iou3d_utils
        iou_of = torch.zeros(rois.shape[0]).type_as(gts)
        for k in range(rois.shape[0]):
            temp_iou = cnt = 0
            roi = rois[k]
            gt = gts[k].view(1, 7)
            aug, keep, tried = roi, True, []
            while temp_iou < self.pos_thresh and cnt < aug_times:
                if self.rng.rand() < KEEP_PROB:
                    aug, keep = roi, True
                else:
                    aug, keep = self._random_aug_box3d(roi), False
                aug = aug.view((1, 7))
                temp_iou = iou3d_utils.boxes_iou3d_gpu(aug, gt)[0][0]
                tried.append(np.float32(temp_iou))
                cnt += 1
            rois[k] = aug.view(-1)
            iou_of[k] = iou_src[k] if cnt == 0 or keep else temp_iou
            rec["cnt"].append(cnt)
            rec["keep"].append(bool(keep))
            rec["tried"].append(tried)
        return rois, iou_of

    def _sample_cpu(self, roi_boxes3d, gt_boxes3d):
        import torch
        from . import iou3d_utils
        R, Rc = self.n_rois, self.cfg.RCNN
        B = roi_boxes3d.size(0)
        batch_rois = gt_boxes3d.new_zeros((B, R, 7))
        batch_gt = gt_boxes3d.new_zeros((B, R, 7))
        batch_iou = gt_boxes3d.new_zeros((B, R))
        for b in range(B):
            cur_roi, cur_gt = roi_boxes3d[b], gt_boxes3d[b]
            k = len(cur_gt) - 1
            while k >= 0 and cur_gt[k].sum() == 0:
                k -= 1
            if k < 0:
                raise ValueError("rcnn_targets: scene %d has no ground-truth box" % b)
            cur_gt = cur_gt[:k + 1]
            iou3d = iou3d_utils.boxes_iou3d_gpu(cur_roi, cur_gt[:, 0:7])
            max_overlaps, gt_assignment = torch.max(iou3d, dim=1)
            lists = [torch.nonzero(max_overlaps >= self.pos_thresh).view(-1),
                     torch.nonzero((max_overlaps < Rc.CLS_BG_THRESH) & (max_overlaps >= Rc.CLS_BG_THRESH_LO)).view(-1),
                     torch.nonzero(max_overlaps < Rc.CLS_BG_THRESH_LO).view(-1)]
            sizes = tuple(int(v.numel()) for v in lists)
            picks, n_fg = self._draw_picks(*sizes)
            chosen = torch.tensor([int(lists[l][p]) for l, p in picks], dtype=torch.long)
            rec = {"sizes": sizes, "lists": [v.numpy().astype(np.int64) for v in lists], "chosen": chosen.numpy().copy(), "n_fg": n_fg,
                   "cnt": [], "keep": [], "tried": [], "iou3d": iou3d.numpy().copy(), "max_overlaps": max_overlaps.numpy().copy()}
            parts = []
            for inds, times in ((chosen[:n_fg], self.aug_times), (chosen[n_fg:], 1 if self.aug_times > 0 else 0)):
                if inds.numel() > 0:
                    gt_of = cur_gt[gt_assignment[inds]]
                    rois, iou = self._aug_rois_cpu(cur_roi[inds], gt_of, max_overlaps[inds], times, rec)
                    parts.append((rois, iou, gt_of))
            batch_rois[b] = torch.cat([p[0] for p in parts], dim=0)
            batch_iou[b] = torch.cat([p[1] for p in parts], dim=0)
            batch_gt[b] = torch.cat([p[2] for p in parts], dim=0)
            rec["cnt"], rec["keep"] = np.array(rec["cnt"], dtype=np.int64), np.array(rec["keep"], dtype=bool)
            self._record.append(rec)
        return batch_rois, batch_gt, batch_iou

    def _augment_cpu(self, pts, rois, gt_of_rois):
        """data_augmentation: rotation, scale, flip of every RoI's cloud and boxes"""
        import torch
        from . import kitti_utils
        B, R = pts.shape[0], pts.shape[1]
        rot = _opt(self.cfg, "AUG_ROT_RANGE", 18)
        angles = (torch.rand((B, R), generator=self.tgen) - 0.5 / 0.5) * (np.pi / rot)          # sic: rand - 1

        def alpha_of(boxes):
            beta = torch.atan2(boxes[:, :, 2], boxes[:, :, 0])
            return -torch.sign(beta) * np.pi / 2 + beta + boxes[:, :, 6]
        gt_alpha, roi_alpha = alpha_of(gt_of_rois), alpha_of(rois)
        for k in range(B):
            pts[k] = kitti_utils.rotate_pc_along_y_torch(pts[k], angles[k])
            gt_of_rois[k] = kitti_utils.rotate_pc_along_y_torch(gt_of_rois[k].unsqueeze(dim=1), angles[k]).squeeze(dim=1)
            rois[k] = kitti_utils.rotate_pc_along_y_torch(rois[k].unsqueeze(dim=1), angles[k]).squeeze(dim=1)
            # (the reference recomputes the headings of ALL scenes in every iteration; the last one's values stay)
            for boxes, alpha in ((gt_of_rois, gt_alpha), (rois, roi_alpha)):
                beta = torch.atan2(boxes[:, :, 2], boxes[:, :, 0])
                boxes[:, :, 6] = torch.sign(beta) * np.pi / 2 + alpha - beta
        scales = 1 + ((torch.rand((B, R), generator=self.tgen) - 0.5) / 0.5) * 0.05
        pts = pts * scales.unsqueeze(dim=2).unsqueeze(dim=3)
        gt_of_rois[:, :, 0:6] = gt_of_rois[:, :, 0:6] * scales.unsqueeze(dim=2)
        rois[:, :, 0:6] = rois[:, :, 0:6] * scales.unsqueeze(dim=2)
        flip_flag = torch.sign(torch.rand((B, R), generator=self.tgen) - 0.5)
        pts[:, :, :, 0] = pts[:, :, :, 0] * flip_flag.unsqueeze(dim=2)
        for boxes in (gt_of_rois, rois):
            boxes[:, :, 0] = boxes[:, :, 0] * flip_flag
            src_ry = boxes[:, :, 6]
            boxes[:, :, 6] = (flip_flag == 1).float() * src_ry + (flip_flag == -1).float() * (torch.sign(src_ry) * np.pi - src_ry)
        return pts, rois, gt_of_rois

    def _forward_cpu(self, d):
        import torch
        from . import kitti_utils, roipool3d_utils
        Rc = self.cfg.RCNN
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        d = {k: t(v) for k, v in d.items()}
        _check_inputs(d, Rc, cuda=False)
        with host_backend():
            batch_rois, batch_gt, batch_iou = self._sample_cpu(d["roi_boxes3d"], d["gt_boxes3d"])
            pts_feature = _point_features(d, Rc)
            pooled, empty = roipool3d_utils.roipool3d_gpu(d["rpn_xyz"], pts_feature, batch_rois, Rc.POOL_EXTRA_WIDTH,
                                                          sampled_pt_num=Rc.NUM_POINTS)
        sampled_pts, sampled_features = pooled[:, :, :, 0:3], pooled[:, :, :, 3:]
        if _opt(self.cfg, "AUG_DATA", True):
            sampled_pts, batch_rois, batch_gt = self._augment_cpu(sampled_pts, batch_rois, batch_gt)
        B = batch_rois.shape[0]
        roi_ry = batch_rois[:, :, 6] % (2 * np.pi)
        roi_center = batch_rois[:, :, 0:3]
        sampled_pts = sampled_pts - roi_center.unsqueeze(dim=2)
        batch_gt[:, :, 0:3] = batch_gt[:, :, 0:3] - roi_center
        batch_gt[:, :, 6] = batch_gt[:, :, 6] - roi_ry
        for k in range(B):
            sampled_pts[k] = kitti_utils.rotate_pc_along_y_torch(sampled_pts[k], batch_rois[k, :, 6])
            batch_gt[k] = kitti_utils.rotate_pc_along_y_torch(batch_gt[k].unsqueeze(dim=1), roi_ry[k]).squeeze(dim=1)
        valid = (empty == 0)
        reg_valid_mask = ((batch_iou > Rc.REG_FG_THRESH) & valid).long()
        cls_label = (batch_iou > Rc.CLS_FG_THRESH).long()
        invalid = (batch_iou > Rc.CLS_BG_THRESH) & (batch_iou < Rc.CLS_FG_THRESH)
        cls_label[valid == 0] = -1
        cls_label[invalid > 0] = -1
        S = Rc.NUM_POINTS
        return {"sampled_pts": sampled_pts.reshape(-1, S, 3), "pts_feature": sampled_features.reshape(-1, S, sampled_features.shape[3]),
                "cls_label": cls_label.view(-1), "reg_valid_mask": reg_valid_mask.view(-1), "gt_of_rois": batch_gt.view(-1, 7),
                "gt_iou": batch_iou.view(-1), "roi_boxes3d": batch_rois.view(-1, 7)}

    # -------------------------------------------------------------------------------------------------------------- device path
    def _pools(self, n_pool):
        """The scene's try pools from the current states, which stay where they were: keep (n_pool) u8, noise (n_pool, 8) f32 --
        row i = what the try at numpy position i reads (level, 7 uniforms) -- and the not-kept flags for the count afterwards"""
        import torch
        D = DRAWS[self.method]
        st_np, st_t = self.rng.get_state(), self.tgen.get_state()
        U = self.rng.rand(n_pool)
        self.rng.set_state(st_np)
        Rp = torch.rand(D * n_pool, generator=self.tgen).numpy()
        self.tgen.set_state(st_t)
        noised = ~(U < KEEP_PROB)
        first = D * (np.cumsum(noised) - noised)                             # the torch position of the try at numpy position i
        noise = np.zeros((n_pool, 8), dtype=np.float32)
        if self.method == "multiple":
            Ip = torch.randint(low=0, high=len(MULTIPLE_RANGES), size=(D * n_pool,), generator=self.tgen).numpy()
            self.tgen.set_state(st_t)
            noise[:, 0] = Ip[first]
            first = first + 1
        for q in range(7):
            noise[:, 1 + q] = Rp[first + q]
        return (~noised).astype(np.uint8), noise, noised

    def _forward_device(self, d):
        import torch
        cfg, Rc, dev = self.cfg, self.cfg.RCNN, self.device
        _check_inputs(d, Rc, cuda=True)
        rois, gt = d["roi_boxes3d"], d["gt_boxes3d"]
        B, M, G, R = rois.shape[0], rois.shape[1], gt.shape[1], self.n_rois
        ntile = (M + 63) // 64
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        max_ov, assign, cls = f32(B, M), i32(B, M), torch.empty((B, M), dtype=torch.uint8, device=dev)
        tile_cnt, lists, sizes = i32(B, 3, ntile), i32(B, 3, M), i32(B, 4)
        stream = C.c_void_p(_lib.current_stream(rois))
        _lib.call("prcnn_rcnn_assign", B, M, G, rois.data_ptr(), gt.data_ptr(), C.c_float(self.pos_thresh), C.c_float(Rc.CLS_BG_THRESH),
                  C.c_float(Rc.CLS_BG_THRESH_LO), max_ov.data_ptr(), assign.data_ptr(), cls.data_ptr(), tile_cnt.data_ptr(),
                  lists.data_ptr(), sizes.data_ptr(), stream)
        sizes_h = sizes.cpu().numpy().astype(np.int64)                       # the batch's one read of B x 4 ints
        self.stats["host_reads"] += 1
        for b in range(B):
            if sizes_h[b, 3] == 0:
                raise ValueError("rcnn_targets: scene %d has no ground-truth box" % b)
        fg_times = self.aug_times if self.pos_thresh > 0 else 0            # `while temp_iou < pos_thresh` with temp_iou = 0
        bg_times = 1 if fg_times > 0 else 0
        W = max(fg_times, 1)
        o_rois, o_pool, o_gt, o_iou = f32(B, R, 7), f32(B, R, 7), f32(B, R, 7), f32(B, R)
        o_src, o_cnt, o_keep, o_tried, used = i32(B, R), i32(B, R), i32(B, R), f32(B, R, W), i32(B)
        table = f32(max(1, R * R * fg_times))
        D = DRAWS[self.method]
        for b in range(B):
            n_fg_list, n_hard, n_easy = (int(v) for v in sizes_h[b, 0:3])
            picks, n_fg = self._draw_picks(n_fg_list, n_hard, n_easy)
            n_pool = n_fg * fg_times + (R - n_fg) * bg_times
            a = _AugArgs(M, G, R, n_fg, fg_times, bg_times, 1 if self.method == "multiple" else 0, n_pool, self.pos_thresh,
                         float(Rc.POOL_EXTRA_WIDTH), rois[b].data_ptr(), gt[b].data_ptr(), max_ov[b].data_ptr(), assign[b].data_ptr(),
                         lists[b].data_ptr(), None, None, None, table.data_ptr(), o_rois[b].data_ptr(), o_pool[b].data_ptr(),
                         o_gt[b].data_ptr(), o_iou[b].data_ptr(), o_src[b].data_ptr(), o_cnt[b].data_ptr(), o_keep[b].data_ptr(),
                         o_tried[b].data_ptr(), used[b:].data_ptr())
            t_pick = torch.tensor(picks, dtype=torch.int32).reshape(R, 2).to(dev)
            a.pick = t_pick.data_ptr()
            if n_pool > 0:
                keep, noise, noised = self._pools(n_pool)
                t_keep, t_noise = torch.from_numpy(keep).to(dev), torch.from_numpy(noise).to(dev)
                a.keep, a.noise = t_keep.data_ptr(), t_noise.data_ptr()
            _lib.call("prcnn_rcnn_aug_rois", C.byref(a), stream)
            if n_pool > 0:
                n_used = int(used[b].item())                                 # the scene's one int: the next scene's draws follow it
                self.stats["host_reads"] += 1
                if not 0 <= n_used <= n_pool:
                    raise _lib.PrcnnError("rcnn_targets: the device used %d of %d draws" % (n_used, n_pool))
                if n_used:
                    self.rng.rand(n_used)
                    n_t = D * int(noised[:n_used].sum())
                    if n_t:
                        torch.rand(n_t, generator=self.tgen)
            self._record.append({"sizes": tuple(int(v) for v in sizes_h[b, 0:3]), "n_fg": n_fg,
                                 "device": {"lists": lists[b], "src": o_src[b], "cnt": o_cnt[b], "keep": o_keep[b], "tried": o_tried[b],
                                            "max_ov": max_ov[b]}})
        aug_data = bool(_opt(cfg, "AUG_DATA", True))
        t_rand = None
        if aug_data:
            t_rand = torch.stack([torch.rand((B, R), generator=self.tgen) for _ in range(3)]).to(dev)
        pts_feature = _point_features(d, Rc).contiguous()
        N, Cf, S = d["rpn_xyz"].shape[1], pts_feature.shape[2], int(Rc.NUM_POINTS)
        pooled = torch.zeros((B, R, S, 3 + Cf), dtype=torch.float32, device=dev)
        empty = torch.zeros((B, R), dtype=torch.int32, device=dev)
        _lib.call("prcnn_roipool3d", B, N, R, Cf, S, d["rpn_xyz"].data_ptr(), o_pool.data_ptr(), pts_feature.data_ptr(), pooled.data_ptr(),
                  empty.data_ptr(), stream)
        out = {"sampled_pts": f32(B * R, S, 3), "pts_feature": f32(B * R, S, Cf),
               "cls_label": torch.empty((B * R,), dtype=torch.int64, device=dev),
               "reg_valid_mask": torch.empty((B * R,), dtype=torch.int64, device=dev), "gt_of_rois": f32(B * R, 7), "gt_iou": o_iou.view(-1),
               "roi_boxes3d": f32(B * R, 7)}
        ta = _TargetArgs(B * R, S, 3 + Cf, int(aug_data), np.pi / _opt(cfg, "AUG_ROT_RANGE", 18), Rc.REG_FG_THRESH, Rc.CLS_FG_THRESH,
                         Rc.CLS_BG_THRESH, pooled.data_ptr(), empty.data_ptr(), None if t_rand is None else t_rand.data_ptr(),
                         o_rois.data_ptr(), o_gt.data_ptr(), o_iou.data_ptr(), out["roi_boxes3d"].data_ptr(), out["gt_of_rois"].data_ptr(),
                         out["sampled_pts"].data_ptr(), out["pts_feature"].data_ptr(), out["cls_label"].data_ptr(),
                         out["reg_valid_mask"].data_ptr())
        _lib.call("prcnn_rcnn_targets", C.byref(ta), stream)
        return out

    def forward(self, input_dict):
        self._record = []
        if self.device == "cpu":
            return self._forward_cpu(input_dict)
        return self._forward_device(input_dict)

    __call__ = forward


def _point_features(d, Rc):
    """[intensity] | seg mask | [depth / 70 - 0.5] | rpn features, as the layer concatenates them before pooling"""
    import torch
    extra = [d["rpn_intensity"].unsqueeze(dim=2)] if Rc.USE_INTENSITY else []
    extra.append(d["seg_mask"].unsqueeze(dim=2))
    if Rc.USE_DEPTH:
        extra.append((d["pts_depth"] / 70.0 - 0.5).unsqueeze(dim=2))
    return torch.cat(extra + [d["rpn_features"]], dim=2)


def _check_inputs(d, Rc, cuda):
    """shapes, dtypes, contiguity: raised here, before any launch"""
    import torch
    keys = ["roi_boxes3d", "gt_boxes3d", "rpn_xyz", "rpn_features", "seg_mask"] + (["pts_depth"] if Rc.USE_DEPTH else []) + \
           (["rpn_intensity"] if Rc.USE_INTENSITY else [])
    for k in keys:
        if k not in d:
            raise ValueError("rcnn_targets: input %r is missing" % k)
        v = d[k]
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or not v.is_contiguous() or v.is_cuda != cuda:
            raise ValueError("rcnn_targets: %s must be a contiguous float32 %s tensor" % (k, "device" if cuda else "CPU"))
    rois, gt, xyz = d["roi_boxes3d"], d["gt_boxes3d"], d["rpn_xyz"]
    if rois.dim() != 3 or rois.shape[2] != 7 or gt.dim() != 3 or gt.shape[2] != 7 or gt.shape[0] != rois.shape[0]:
        raise ValueError("rcnn_targets: roi_boxes3d %s / gt_boxes3d %s" % (tuple(rois.shape), tuple(gt.shape)))
    B = rois.shape[0]
    if rois.shape[1] == 0 or gt.shape[1] == 0:
        raise ValueError("rcnn_targets: no RoI or no ground-truth box (M = %d, G = %d)" % (rois.shape[1], gt.shape[1]))
    if xyz.dim() != 3 or xyz.shape[0] != B or xyz.shape[2] != 3:
        raise ValueError("rcnn_targets: rpn_xyz %s" % (tuple(xyz.shape),))
    N = xyz.shape[1]
    if d["rpn_features"].dim() != 3 or tuple(d["rpn_features"].shape[0:2]) != (B, N):
        raise ValueError("rcnn_targets: rpn_features %s" % (tuple(d["rpn_features"].shape),))
    for k in keys[4:]:
        if tuple(d[k].shape) != (B, N):
            raise ValueError("rcnn_targets: %s %s, expected %s" % (k, tuple(d[k].shape), (B, N)))
    if int(Rc.NUM_POINTS) < 1:
        raise ValueError("rcnn_targets: RCNN.NUM_POINTS %r" % (Rc.NUM_POINTS,))
