"""The runners of the evaluation harness and the final stage they call: how a batch's stages (geometry, RPN stage, proposal layer,
RCNN features, final stage) are put onto HIP streams -- enqueued eagerly (PipelinedRunner) or replayed from hipGraphs (GraphedRunner) --
and the serial runners for configurations those two do not cover.  eval_rcnn.py drives them and re-exports every name."""
import collections
import contextlib
import os

import torch

from . import kitti_utils
from . import iou3d_utils
from .bbox_transform import decode_bbox_target
from .net.fast_infer import FastPointRCNN
from ._lib import has_entry

# (removed in round 4, results in DESIGN.md section 7: PRCNN_GEO_THREAD -- geometry chains enqueued by a helper thread, slower: the GIL;
#  PRCNN_RCNN_GEO_STREAM -- the RCNN's geometry on a stream of its own, slower: a 5th busy stream shares a hardware queue; PRCNN_GATE --
#  chains only started at the end of an RPN stage, slower since the stages are our own ticketed kernels; PRCNN_STREAM_SKEW)


_ANCHORS = {}
FUSED_POSTPROCESS = True     # final stage through the fused HIP entry when the extension offers it
# Round 4: the final stage (decode + threshold + rotated NMS, 0.2 ms) runs BEHIND the RCNN features on the feature stream instead of
# on the proposal stream: with the FP modules on the geometry streams (fast_infer.EARLY_FP = 3) the proposal stream -- proposal layer,
# RoI pooling, the RoI clouds' geometry, final stage -- was the longest of the four, and the hop feature -> proposal -> host costs two
# event waits.  Round 5, second session: back on the proposal stream by default -- with the pack launches, half of the RoI geometry and the
# padded tiles gone that stream is busy 0.35-0.40 ms of a 0.97-ms step and the feature stream is the fullest (0.78): K = 20 7253 / 7238 /
# 7226 -> 7323 / 7261 / 7256 scenes/s, LiDAR-shaped 5109 / 5134 / 5143 -> 5183 / 5175 / 5180 (three alternating runs of five windows each);
# K = 100 unchanged.
# batches of a geometry group that share the launches of the stages behind the geometry in the graphed runner (GraphedRunner.pair):
# 2 (measured: 6040-6150 / 6980-7050 scenes/s at K = 20 / 100 against 5800-5860 / 6730-6750 with 1, LiDAR-shaped 4270-4350 / 4930-4970
# against 4140-4160 / 4830; 4: 6060 / 6780 and 4330 / 4750); 1: every batch its own launches
RCNN_PAIR = int(os.environ.get("PRCNN_PAIR", "2"))


def _anchor_host(cfg):
    """CLS_MEAN_SIZE rounded to f32, as python floats (h, w, l)."""
    import numpy as np
    return [float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32)]


def _anchor_on(cfg, device):
    """CLS_MEAN_SIZE as a device tensor, uploaded once (a per-call H2D copy synchronises the stream)."""
    key = (str(device), tuple(float(v) for v in cfg.CLS_MEAN_SIZE[0]))
    if key not in _ANCHORS:
        _ANCHORS[key] = torch.tensor(key[1], dtype=torch.float32, device=device)
    return _ANCHORS[key]


def split_detections(blob, batch_size, M):
    """blob (batch_size * (8 M + 1)) f32, device or host -> views boxes (B,M,7) f32, scores (B,M) f32, num (B) i32 (the same bytes)."""
    nb, ns = batch_size * M * 7, batch_size * M
    return (blob[:nb].view(batch_size, M, 7), blob[nb:nb + ns].view(batch_size, M), blob[nb + ns:nb + ns + batch_size].view(torch.int32))


@torch.no_grad()
def postprocess(cfg, ret_dict, batch_size, blob_scenes=None):
    """Final box decoding + score threshold + rotated NMS, batched (eval_rcnn.py:506-530,611-629).
    Returns boxes (B,M,7), raw scores (B,M) and num (B) i32 on the device; rows >= num are zero.
    blob_scenes (the graphed runner's launches over several batches): the results as one blob per `blob_scenes` scenes --
    "blobs" (B / blob_scenes, blob_scenes (8 M + 1)); boxes / scores / num are then LISTS of per-blob views."""
    R = cfg.RCNN
    rois = ret_dict["rois"]
    M = rois.shape[1]
    rcnn_cls = ret_dict["rcnn_cls"].view(batch_size, M, -1)
    rcnn_reg = ret_dict["rcnn_reg"].view(batch_size, M, -1)
    if rcnn_cls.shape[2] != 1:
        raise NotImplementedError("multi-class RCNN head")
    raw = rcnn_cls[:, :, 0]
    ext = iou3d_utils.iou3d_cuda
    if FUSED_POSTPROCESS and M <= 128 and has_entry(ext, "rcnn_postprocess"):
        # one extension call (three launches): decode, threshold, score sort, rotated NMS, assembly
        dev = rois.device
        pred = torch.empty((batch_size, M, 7), dtype=torch.float32, device=dev)
        # the three results in ONE allocation ("blob": boxes | scores | num, see split_detections): the consumer brings them to the host
        # with one copy instead of three
        raw = raw.contiguous()
        if blob_scenes and blob_scenes < batch_size and batch_size % blob_scenes == 0 and has_entry(ext, "rcnn_postprocess_blobs") and R.NMS_THRESH >= 0:
            nb = batch_size // blob_scenes
            blobs = torch.empty((nb, blob_scenes * (M * 8 + 1)), dtype=torch.float32, device=dev)
            ext.rcnn_postprocess_blobs(rois.contiguous(), rcnn_reg.contiguous(), raw, _anchor_host(cfg), R.LOC_SCOPE, R.LOC_BIN_SIZE,
                                       R.NUM_HEAD_BIN, R.LOC_Y_BY_BIN, R.LOC_Y_SCOPE, R.LOC_Y_BIN_SIZE, R.SCORE_THRESH, R.NMS_THRESH,
                                       pred, blobs, blob_scenes)
            parts = [split_detections(blobs[i], blob_scenes, M) for i in range(nb)]
            return {"boxes": [p[0] for p in parts], "scores": [p[1] for p in parts], "num": [p[2] for p in parts], "pred_boxes3d": pred,
                    "raw_scores": raw, "blobs": blobs}
        blob = torch.empty((batch_size * (M * 8 + 1),), dtype=torch.float32, device=dev)
        boxes, scores, num = split_detections(blob, batch_size, M)
        ext.rcnn_postprocess(rois.contiguous(), rcnn_reg.contiguous(), raw, _anchor_host(cfg), R.LOC_SCOPE,
                             R.LOC_BIN_SIZE, R.NUM_HEAD_BIN, R.LOC_Y_BY_BIN, R.LOC_Y_SCOPE, R.LOC_Y_BIN_SIZE,
                             R.SCORE_THRESH, R.NMS_THRESH, pred, boxes, scores, num)
        return {"boxes": boxes, "scores": scores, "num": num, "pred_boxes3d": pred, "raw_scores": raw, "blob": blob}
    anchor = _anchor_on(cfg, rois.device)
    pred = decode_bbox_target(rois.view(-1, 7), rcnn_reg.view(-1, rcnn_reg.shape[-1]), anchor_size=anchor,
                              loc_scope=R.LOC_SCOPE, loc_bin_size=R.LOC_BIN_SIZE, num_head_bin=R.NUM_HEAD_BIN,
                              get_xz_fine=True, get_y_by_bin=R.LOC_Y_BY_BIN, loc_y_scope=R.LOC_Y_SCOPE,
                              loc_y_bin_size=R.LOC_Y_BIN_SIZE, get_ry_fine=True).view(batch_size, M, 7)
    selected = torch.sigmoid(raw) > R.SCORE_THRESH
    if not hasattr(ext, "nms_device"):
        # the reference's four entry points only (compiled dropin_native/iou3d_cuda): scene by scene over the blocking nms_gpu,
        # as eval_rcnn.py:611-629
        boxes, scores = torch.zeros_like(pred), torch.zeros_like(raw)
        num = torch.zeros((batch_size,), dtype=torch.int32, device=raw.device)
        for k in range(batch_size):
            cur = selected[k]
            if int(cur.sum()) == 0:
                continue
            b_sel, s_sel = pred[k][cur], raw[k][cur]
            keep = iou3d_utils.nms_gpu(kitti_utils.boxes3d_to_bev_torch(b_sel), s_sel, R.NMS_THRESH)
            boxes[k, :keep.numel()] = b_sel[keep]
            scores[k, :keep.numel()] = s_sel[keep]
            num[k] = keep.numel()
        return {"boxes": boxes, "scores": scores, "num": num, "pred_boxes3d": pred, "raw_scores": raw}
    key = torch.where(selected, raw, torch.full_like(raw, float("-inf")))
    _, order = torch.sort(key, dim=1, descending=True)          # selected boxes first, by raw score
    counts = selected.sum(dim=1).to(torch.int32)
    boxes_sorted = torch.gather(pred, 1, order.unsqueeze(-1).expand(-1, -1, 7))
    scores_sorted = torch.gather(raw, 1, order)
    bev = kitti_utils.boxes3d_to_bev_torch(boxes_sorted.reshape(-1, 7)).view(batch_size, M, 5)
    keep, num = iou3d_utils.nms_device_batched(bev, counts, R.NMS_THRESH, True, M)
    valid = torch.arange(M, device=raw.device).unsqueeze(0) < num.long().unsqueeze(1)
    rows = keep.long().clamp(min=0)
    boxes = torch.gather(boxes_sorted, 1, rows.unsqueeze(-1).expand(-1, -1, 7)) * valid.unsqueeze(-1)
    scores = torch.gather(scores_sorted, 1, rows) * valid
    return {"boxes": boxes, "scores": scores, "num": num, "pred_boxes3d": pred, "raw_scores": raw}


@torch.no_grad()
def infer_batch(model, cfg, pts_input, engine=None, geo=None):
    """pts_input (B,N,3) device f32 -> detections dict (all device tensors, fixed shapes).
    ``engine`` = a FastPointRCNN built from ``model`` (point-major fused path); without it the
    nn.Module graph (reference operation order) runs."""
    ret = engine(pts_input, geo, want_reg=False) if engine is not None else model({"pts_input": pts_input})
    det = postprocess(cfg, ret, pts_input.shape[0])
    det["rois"] = ret["rois"]
    det["rcnn_reg"] = ret["rcnn_reg"]
    det["rcnn_cls"] = ret["rcnn_cls"]
    return det


_RUNNER_STREAMS = {}


def _runner_streams(device, n_sides, prio):
    """The side / tail streams of the pipelined runner, created ONCE per (device, priority) and shared by every runner of the
    process.  HIP multiplexes its streams onto a few hardware queues (4 by default); two streams that land on the same queue
    serialise -- a feature-stream kernel then waits behind a 6 ms FPS kernel of a geometry chain.  A fresh set of streams
    per runner drew a new mapping every time (same process: 77 ms or 89 ms for the same 20 steps); with one fixed set the
    first-created streams keep the queues they were given at start-up."""
    key = (str(device), prio)
    have = _RUNNER_STREAMS.setdefault(key, {"tail": None, "sides": [], "feat": None})
    if have["tail"] is None:
        have["tail"] = torch.cuda.Stream(device)
    while len(have["sides"]) < n_sides:
        have["sides"].append(torch.cuda.Stream(device, priority=prio))
    return have["tail"], have["sides"][:n_sides]


class _StagedRunner:
    """What the two staged runners -- eager enqueue (PipelinedRunner) and graph replay (GraphedRunner) -- share: the engine, the
    streams, the look-ahead knobs and the rules that decide when the geometry chain of the next group of batches starts."""

    def __init__(self, model, cfg, device, depth=None):
        self.model, self.cfg = model, cfg
        self.engine = FastPointRCNN(model, cfg)
        self.device = torch.device(device)
        # geometry runs for GROUPS of `group` batches in one chain (FastPointRCNN.geometry_group): a scene's FPS is serial
        # (~6.8 ms for 16384 -> 4096 on one CU) whatever the batch, so one chain over 3 batches costs the latency of one and
        # a single chain in flight keeps up with the feature stream.  `depth` = how many batches ahead the caller should
        # hand over (3 * group: a chain is launched 2 * `group` steps before its first batch is due; with 2 * group the chain -- 7 ms alone,
        # 11 ms beside the feature stream -- was just late for the first batch of every group: +0.5 ms once per group).
        self.group = max(1, int(os.environ.get("PRCNN_GEO_GROUP", "4")))
        self.depth = self.default_depth() if depth is None else depth
        # default priority: with the SA levels on the packed MFMA kernels the feature pass is short, and high-priority side
        # streams (three of them at depth 3) starve it -- measured 971 vs 1375 scenes/s (the switch PRCNN_SIDE_PRIORITY is gone, round 6)
        self.tail, self.sides = _runner_streams(self.device, int(os.environ.get("PRCNN_SIDE_STREAMS", "2")), 0)

    @staticmethod
    def default_depth():
        """Batches of look-ahead a caller should hand over (PRCNN_GEO_DEPTH; 3 x PRCNN_GEO_GROUP by default)."""
        group = max(1, int(os.environ.get("PRCNN_GEO_GROUP", "4")))
        return int(os.environ.get("PRCNN_GEO_DEPTH", str(3 * group)))

    def _look_ahead(self, upcoming):
        """``upcoming`` (None, a batch, or a list of batches with None at the end of a run) -> list of at most `depth` batches"""
        todo = [] if upcoming is None else (list(upcoming) if isinstance(upcoming, (list, tuple)) else [upcoming])
        return [p for p in todo if p is not None][:max(1, self.depth)]

    def _next_group_due(self, todo, missing, ending=False):
        """Start the next chain now?  `missing` = the batches of the look-ahead `todo` that have no chain yet: as soon as a whole
        group of them has none (with a look-ahead of 2 * group that is `group` steps before its first batch is due), or when the
        look-ahead is about to run dry (or, the caller says, the run is `ending`)."""
        have = len(todo) - len(missing)
        return bool(missing) and (len(missing) >= self.group or have <= 1 or ending)

    def drain(self):
        """flush() until the pipeline is empty: the detections of every batch not handed back yet, oldest first (probes and
        timing loops call this in front of a synchronize -- ONE flush() leaves up to two batches' RCNN + final stages unlaunched)."""
        out = []
        while True:
            det = self.flush()
            if det is None:
                return out
            out.append(det)

    def _role_streams(self):
        """every stream besides the caller's that runs the engine for this runner"""
        return [self.tail] + list(self.sides)

    def _reload_ordered(self):
        """engine.reload_weights() on the caller's stream, behind everything the role streams still run with the old weights (geometry
        chains of batches that were announced and never submitted: their early SA levels read the weights) and in front of
        everything they run next: ONE event recorded behind the refresh, waited for by each of them."""
        main = torch.cuda.current_stream(self.device)
        for s in self._role_streams():
            main.wait_stream(s)
        self.engine.reload_weights()
        ev = torch.cuda.Event()
        ev.record(main)
        for s in self._role_streams():
            s.wait_event(ev)


# a batch between its RPN stage and its RCNN stage (PipelinedRunner._inflight): its clouds, the RPN stage's state, the proposal layer's
# results and the event behind them, the side stream that owns its geometry, that geometry, the RCNN geometry
_InFlight = collections.namedtuple("_InFlight", "pts st rois roi_scores ev_prop side geo rg")


class PipelinedRunner(_StagedRunner):
    """Software pipeline over batches on HIP streams: the xyz-only GEOMETRY of upcoming batches (FPS,
    ball query, three-NN: a latency-bound chain that keeps only B CUs busy) runs on side streams while
    the FEATURE pass of the current batch (MFMA kernels, GEMMs, pooling, NMS) fills the rest of the chip
    on the main stream.  ``depth`` batches of geometry are kept in flight.
    Call ``step(cur, upcoming)`` once per batch; ``upcoming`` = the next batch, or a list of the next
    ``depth`` batches, or None at the end."""

    def __init__(self, model, cfg, device, depth=None):
        super().__init__(model, cfg, device, depth)
        self._next_side = 0
        self._pending = []        # step(): [(batch tensor, geometry dict, ready event)] in launch order
        self._inflight = None     # submit(): the batch whose RCNN stage is still to come (_InFlight)
        self._chains = []         # geometry chains launched for batches not submitted yet: dicts pts / side / geo / ev
        self._retired = []        # (side stream, RCNN-done event, geometry) of batches whose geometry is still kept

    @property
    def side(self):
        return self.sides[0]

    def _launch_geometry(self, pts):
        main = torch.cuda.current_stream(self.device)
        side = self.sides[self._next_side % len(self.sides)]
        self._next_side += 1
        side.wait_stream(main)                        # pts (and the allocator's frees) are ordered before us
        with torch.cuda.stream(side):
            geo = self.engine.geometry(pts)
            ev = torch.cuda.Event()
            ev.record(side)
        for t in _tensors(geo):                       # consumed on the main stream: tell the caching allocator
            t.record_stream(main)
        self._pending.append((pts, geo, ev))

    def _take(self, pts):
        for i, (p, geo, ev) in enumerate(self._pending):
            if p is pts:
                del self._pending[i]
                return geo, ev
        self._launch_geometry(pts)
        return self._take(pts)

    def _prefetch_geometry(self, upcoming):
        if upcoming is not None:
            todo = list(upcoming) if isinstance(upcoming, (list, tuple)) else [upcoming]
            for nxt in todo[:max(1, self.depth)]:
                if nxt is not None and all(p is not nxt for p, _, _ in self._pending):
                    self._launch_geometry(nxt)        # enqueue first: it overlaps the feature pass below

    @torch.no_grad()
    def step(self, cur, upcoming=None):
        geo, ev = self._take(cur)
        self._prefetch_geometry(upcoming)
        torch.cuda.current_stream(self.device).wait_event(ev)
        return infer_batch(self.model, self.cfg, cur, engine=self.engine, geo=geo)

    # ---- three-stream form: the latency-bound tails leave the GEMM stream -------------------------
    # The proposal layer (per-scene score sort, band selection, NMS: ONE workgroup per scene) and the final
    # stage (decode + NMS) keep only B CUs busy.  On the feature stream they would stall the chip-filling
    # kernels behind them, so they run on a third stream and the feature stream is software-pipelined:
    #     feature stream :  RPN(i)   RCNN(i-1)   RPN(i+1)   RCNN(i)   ...
    #     tail stream    :        proposals(i)  final(i-1)      proposals(i+1)  final(i) ...
    #     geometry stream:  geometry(i+1 .. i+group)              geometry(i+group+1 ..)
    # Exactly one stream carries library GEMMs (two GEMM streams deadlock).
    # ``submit`` returns the detections of the PREVIOUS batch (None on the first call), ``flush`` the last one;
    # the returned tensors are produced on ``self.tail``: read them under that stream or after ``det["ready"]``.
    @torch.no_grad()
    def submit(self, cur, upcoming=None):
        main = torch.cuda.current_stream(self.device)
        todo = self._look_ahead(upcoming)
        ch = self._chain(cur)
        if ch is None:                                # cold start (or a caller that looks less far ahead): chain for what is known
            self._launch_group([cur] + [p for p in todo if self._chain(p) is None][:self.group - 1], urgent=True)
            ch = self._chain(cur)
        self._chains = [c for c in self._chains if c is not ch]      # by identity (dict equality would compare tensors)
        missing = [p for p in todo if self._chain(p) is None]
        if self._next_group_due(todo, missing):
            self._launch_group(missing[:self.group])
        main.wait_event(ch["ev"])
        st = self.engine.rpn_stage(cur, ch["geo"])
        ev_rpn = torch.cuda.Event()
        ev_rpn.record(main)
        for t in (st["rpn_scores_raw"], st["rpn_reg"], st.get("rpn_boxes"), st["backbone_xyz"]):
            if t is not None:
                t.record_stream(self.tail)
        rois, roi_scores, ev_prop, rg = self._propose_on_tail(st, ev_rpn)
        done = self._finish_inflight()
        self._inflight = _InFlight(cur, st, rois, roi_scores, ev_prop, ch["side"], ch["geo"], rg)
        return done

    def _propose_on_tail(self, st, ev_rpn):
        """Proposal layer of the batch whose RPN stage ends at `ev_rpn`, on the tail stream -- and right behind it the part of
        its RCNN stage that needs the RoIs and coordinates only (RoI pooling, FPS, ball queries, row lists: ten latency-bound
        launches, 0.3 ms of every step while they sat on the feature stream in front of the RCNN's MFMA kernels).
        -> rois, scores, event (RoIs and the RCNN geometry are ready), RCNN geometry state."""
        with torch.cuda.stream(self.tail):
            self.tail.wait_event(ev_rpn)
            rois, roi_scores = self.engine.propose(st)
            # reads st["rpn_features"] (feature-stream memory: st stays referenced until the feature stream has run this
            # batch's RCNN stage, which waits for ev_prop) and makes ~15 tensors on the tail stream that the feature stream
            # reads: they are kept in self._inflight until the tail stream has waited for that RCNN stage (_finish_inflight)
            rg = self.engine.rcnn_geometry(st, rois)
            ev_prop = torch.cuda.Event()
            ev_prop.record(self.tail)
        return rois, roi_scores, ev_prop, rg

    # ---- geometry: ONE chain per `group` batches (PRCNN_GEO_GROUP=1: per batch) ---------------------------------
    def _launch_group(self, batch_list, urgent=False):
        main = torch.cuda.current_stream(self.device)
        side = self.sides[self._next_side % len(self.sides)]
        self._next_side += 1
        side.wait_stream(main)                        # the batches (and the allocator's frees) are ordered before the chain
        # Geometry tensors are allocated on a side stream and read by the RPN stage on the feature stream.  record_stream()
        # would make that safe, but the caching allocator then records one event ON THE FEATURE STREAM per tensor when the
        # batch's ~40 tensors are freed: 40 marker packets = 0.2 ms of feature-stream time per step (profiles/gap_probe.py,
        # HIP API trace).  Instead a batch's tensors are KEPT (self._retired) until the side stream that owns their memory has
        # been made to wait for the RPN stage that read them -- here, before that stream allocates again.
        mine = [r for r in self._retired if r[0] is side]
        self._retired = [r for r in self._retired if r[0] is not side]
        for _, ev_read, _ in mine:
            side.wait_event(ev_read)
        del mine
        evs = []

        def mark(_):                                  # one event per batch: its RPN stage need not wait for the rest of the group
            e = torch.cuda.Event()
            e.record(side)
            evs.append(e)
        with torch.cuda.device(self.device), torch.cuda.stream(side):
            # urgent (cold start: the first batch of this group is waited for right now): SA levels batch by batch, so that batch 0
            # is ready before the other three are computed; otherwise over the group's clouds at once (a quarter of the launches)
            geos = self.engine.geometry_group(batch_list, on_batch_done=mark, group_sa=not urgent)
            if len(evs) != len(geos):
                ev = torch.cuda.Event()
                ev.record(side)
                evs = [ev] * len(geos)
        self._chains.extend({"pts": pts, "geo": geo, "ev": ev, "side": side} for pts, geo, ev in zip(batch_list, geos, evs))

    def _chain(self, pts):
        for c in self._chains:
            if c["pts"] is pts:
                return c
        return None

    def _finish_inflight(self):
        if self._inflight is None:
            return None
        main = torch.cuda.current_stream(self.device)
        f, self._inflight = self._inflight, None
        main.wait_event(f.ev_prop)
        out = self.engine.rcnn_features(f.rg)
        ev_rcnn = torch.cuda.Event()
        ev_rcnn.record(main)
        # the batch's geometry (read by its RPN stage, its spatial groups by this RCNN stage) retires: kept until the side
        # stream that owns the memory has been made to wait for this point (see _launch_group)
        self._retired.append((f.side, ev_rcnn, f.geo))
        for t in (out["rcnn_cls"], out["rcnn_reg"]):
            t.record_stream(self.tail)
        with torch.cuda.stream(self.tail):
            self.tail.wait_event(ev_rcnn)
            ret = {"rois": f.rois, "rcnn_cls": out["rcnn_cls"], "rcnn_reg": out["rcnn_reg"]}
            det = postprocess(self.cfg, ret, f.pts.shape[0])
            det.update(ret)
            ready = torch.cuda.Event()
            ready.record(self.tail)
        del f                                         # (f.rg: tail-stream memory, read on the feature stream up to ev_rcnn: the tail stream waits for it above)
        det["ready"] = ready
        det["stream"] = self.tail
        return det

    @torch.no_grad()
    def flush(self):
        """Finish the batch still in flight (RCNN + final stage) and return its detections (or None)."""
        det = self._finish_inflight()
        for side, ev_read, _ in self._retired:        # the kept geometry goes back to its streams' pools, ordered after its readers
            side.wait_event(ev_read)
        self._retired = []
        return det

    @torch.no_grad()
    def reload_weights(self):
        """The model's weights were changed on purpose (the next checkpoint of a sweep): FastPointRCNN.reload_weights(), ordered
        against the side and tail streams.  RuntimeError while a batch is in flight -- flush() first.  Geometry chains of batches that
        were announced and not submitted are dropped (their early SA levels were computed with the old weights)."""
        if self._inflight is not None:
            raise RuntimeError("PipelinedRunner.reload_weights: a batch is in flight; flush() first")
        self._chains, self._pending = [], []
        self._reload_ordered()


USE_GRAPHS = os.environ.get("PRCNN_GRAPHS", "1") != "0"                   # hipGraph replay of the stages (GraphedRunner); 0: eager enqueue (PipelinedRunner)


_GRAPH_DEBUG = int(os.environ.get("PRCNN_GRAPH_DEBUG", "0"))   # 1: device sync before a geometry graph, 2: after it (bisecting overlaps)


def engine_covers(cfg):
    """Does the point-major engine (net/fast_infer.py) cover this configuration?  Round 4: cfg.RPN.USE_INTENSITY (a 4-channel
    pts_input, rpn.py:17 / kitti_rcnn_dataset.py:321-338; the reference's code default, lib/config.py:40) runs on the engine too --
    on its general kernels, serially (EngineRunner); the stream-pipelined / graph-replayed runners are written for the (B, N, 3)
    clouds of the shipped configurations.  cfg.RCNN.USE_INTENSITY stays on the nn.Module graph (ModuleRunner)."""
    return not bool(cfg.RCNN.ENABLED and cfg.RCNN.USE_INTENSITY)


_NATIVE_MODULES = None


def native_modules():
    """The three COMPILED extension modules (dropin_native/: pybind11 over the C ABI, the reference's 9 + 4 + 4 entry points and
    nothing else), loaded once from their directory without shadowing the ctypes modules of the same names."""
    global _NATIVE_MODULES
    if _NATIVE_MODULES is None:
        import importlib.util
        from . import NATIVE_DROPIN_DIR
        mods = []
        for name in ("pointnet2_cuda", "iou3d_cuda", "roipool3d_cuda"):
            hits = [f for f in os.listdir(NATIVE_DROPIN_DIR) if f.startswith(name + ".") and f.endswith(".so")]
            if not hits:
                raise RuntimeError("%s: compiled module %s not built (python __graft_entry__.py)" % (NATIVE_DROPIN_DIR, name))
            spec = importlib.util.spec_from_file_location(name, os.path.join(NATIVE_DROPIN_DIR, hits[0]))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
        _NATIVE_MODULES = tuple(mods)
    return _NATIVE_MODULES


@contextlib.contextmanager
def reference_api_only(native=True):
    """What a user of the reference's Python gets from the drop-in modules: inside this context the nn.Module graph runs in the
    reference's operation order over the reference's 17 entry points ONLY -- FPS -> gather -> ball_query -> group (x2) ->
    subtract -> cat -> Conv2d / BatchNorm / ReLU modules -> max_pool2d (pointnet2_modules.py:19-55), three_nn -> three_interpolate
    -> cat -> Conv (:139-151), the per-scene proposal layer and final stage over the blocking nms_gpu / nms_normal_gpu, roipool3d
    forward -- no fused entry, no folded MLP, no engine.  ``native``: through the compiled dropin_native modules (default) or the
    ctypes ones."""
    from .pointnet2 import pointnet2_utils as pu, fused_mlp
    from . import roipool3d_utils as ru
    saved = (pu.pointnet2, iou3d_utils.iou3d_cuda, ru.roipool3d_cuda, pu.REFERENCE_ORDER, fused_mlp.ENABLED)
    if native:
        pu.pointnet2, iou3d_utils.iou3d_cuda, ru.roipool3d_cuda = native_modules()
    else:
        class _Only:
            def __init__(self, mod, names):
                for n in names:
                    setattr(self, n, getattr(mod, n))
        pu.pointnet2 = _Only(pu.pointnet2, ("ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper",
                                            "gather_points_wrapper", "gather_points_grad_wrapper", "furthest_point_sampling_wrapper",
                                            "three_nn_wrapper", "three_interpolate_wrapper", "three_interpolate_grad_wrapper"))
        iou3d_utils.iou3d_cuda = _Only(iou3d_utils.iou3d_cuda, ("boxes_overlap_bev_gpu", "boxes_iou_bev_gpu", "nms_gpu", "nms_normal_gpu"))
        ru.roipool3d_cuda = _Only(ru.roipool3d_cuda, ("forward", "forward_slow", "pts_in_boxes3d_cpu", "roipool3d_cpu"))
    pu.REFERENCE_ORDER, fused_mlp.ENABLED = True, False
    try:
        yield
    finally:
        pu.pointnet2, iou3d_utils.iou3d_cuda, ru.roipool3d_cuda, pu.REFERENCE_ORDER, fused_mlp.ENABLED = saved


class ModuleRunner:
    """submit() / flush() of the pipelined runners over the nn.Module graph (the reference's operation order, HIP operators through the
    drop-in modules, no side streams): for configurations the point-major engine does not cover.  Same one-batch-late protocol."""
    depth = 1

    def __init__(self, model, cfg, device, depth=None):
        self.model, self.cfg, self.device = model, cfg, torch.device(device)
        self._pending = None

    @torch.no_grad()
    def submit(self, cur, upcoming=None):
        done = self._pending
        det = self._infer(cur)
        if self.device.type == "cuda":
            stream = torch.cuda.current_stream(self.device)
            det["ready"] = torch.cuda.Event()
            det["ready"].record(stream)
            det["stream"] = stream
        self._pending = det
        return done

    def flush(self):
        done, self._pending = self._pending, None
        return done

    def drain(self):
        """flush() until the pipeline is empty: the detections of every batch not handed back yet, oldest first (probes and
        timing loops call this in front of a synchronize -- ONE flush() leaves up to two batches' RCNN + final stages unlaunched)."""
        out = []
        while True:
            det = self.flush()
            if det is None:
                return out
            out.append(det)

    def _infer(self, cur):
        return infer_batch(self.model, self.cfg, cur)

    def reload_weights(self):
        """The model's weights were changed on purpose: the engine, where the runner has one, folds them again in place
        (FastPointRCNN.reload_weights; the nn.Module graph reads the model itself).  RuntimeError while a batch is in flight --
        flush() first.  Everything runs on the caller's stream: no ordering is needed."""
        if self._pending is not None:
            raise RuntimeError("%s.reload_weights: a batch is in flight; flush() first" % type(self).__name__)
        if getattr(self, "engine", None) is not None:
            self.engine.reload_weights()


class EngineRunner(ModuleRunner):
    """The same protocol over the point-major engine, one batch after the other on the caller's stream: configurations the
    engine covers on its general kernels only (cfg.RPN.USE_INTENSITY)."""

    def __init__(self, model, cfg, device, depth=None):
        super().__init__(model, cfg, device, depth)
        self.engine = FastPointRCNN(model, cfg)

    def _infer(self, cur):
        return infer_batch(self.model, self.cfg, cur, engine=self.engine)


class RpnRunner(ModuleRunner):
    """--eval_mode rpn (cfg.RCNN.ENABLED = False): the engine's RPN stage and proposal layer, one batch after the other on the caller's
    stream, with the same one-batch-late protocol.  A batch's dict holds rois / roi_scores_raw (B, M, 7) / (B, M), the raw scores
    (B, N), the backbone's xyz (B, N, 3) and its point-major features (B, N, C)."""

    def __init__(self, model, cfg, device, depth=None):
        super().__init__(model, cfg, device, depth)
        if cfg.RCNN.ENABLED:
            raise ValueError("RpnRunner: cfg.RCNN.ENABLED must be False (--eval_mode rpn)")
        self.engine = FastPointRCNN(model, cfg)

    def _infer(self, cur):
        st = self.engine.rpn_stage(cur)
        rois, roi_scores = self.engine.propose(st)
        return {"rois": rois, "roi_scores_raw": roi_scores, "rpn_scores_raw": st["rpn_scores_raw"],
                "backbone_xyz": st["backbone_xyz"], "rpn_features": st["rpn_features"]}


def make_runner(model, cfg, device, depth=None):
    """The runner of the product path: hipGraph replay unless PRCNN_GRAPHS=0 (same streams, same kernels, same results).
    --eval_mode rpn (RCNN disabled): RpnRunner."""
    if not cfg.RCNN.ENABLED:
        return RpnRunner(model, cfg, device, depth)
    if not engine_covers(cfg):
        return ModuleRunner(model, cfg, device, depth)
    if cfg.RPN.USE_INTENSITY:
        return EngineRunner(model, cfg, device, depth)
    from . import GRAPH_REPLAY_SAFE
    if USE_GRAPHS and not GRAPH_REPLAY_SAFE:
        import warnings
        warnings.warn("hipGraph replay disabled: the HIP runtime was initialised before DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 could be set "
                      "(import the package, or export the variable, before the first torch.cuda call); using the eager runner")
    return (GraphedRunner if USE_GRAPHS and GRAPH_REPLAY_SAFE else PipelinedRunner)(model, cfg, device, depth)


class GraphedRunner(_StagedRunner):
    """PipelinedRunner with every stage captured ONCE into a hipGraph and replayed: the same kernels with the same arguments on the
    same streams in the same order -- the host's part of a step falls from ~70 extension calls + their torch glue (0.8 ms of Python
    per step, more than half of the step's period: the host thread was co-limiting, profiles/r03_microbench.md) to four graph
    launches and a dozen event operations.

    A graph replays fixed addresses, so the pipeline runs over SLOTS instead of freshly allocated tensors:
      * a group slot holds the coordinates of `group` batches (copied in when their chain is launched: 1.5 MB per batch), the
        geometry graph of the group (FastPointRCNN.geometry_group: FPS / ball queries / row lists / three-NN / the early SA levels,
        on a side stream) and, per MEMBER of the group (`pair` consecutive batches: 2 by default), four graphs: RPN stage (feature
        stream), proposal layer + RCNN geometry (tail stream), RCNN features (feature stream), final stage (behind them on the tail
        stream) -- pair x B scenes per launch of each;
      * depth / group + 1 group slots rotate: a slot is rewritten only after the RCNN stages of its previous batches (an event wait
        on the side stream, normally long past);
      * submit() hands back the detections of an EARLIER batch, in submit order, or None (a member's stages are launched when its
        last batch is submitted, its RCNN + final stages behind the next member's RPN stage: up to 2 pair - 1 submits late); flush()
        one batch per call until None.  They are views into the slot: valid for (slots - 1) * group - 2 pair further submits (8 by
        default) -- copy them out (on det["stream"]) before that, as eval_scenes and bench.py do right away.
    Every graph has a memory pool of its own (see _build); everything a later graph or the caller reads is kept referenced here.  Batches of another shape than the first one seen (the last, short batch of a split) run eagerly.
    Nondeterminism is that of the eager path: the worklists built with atomics (point groups, pooled tiles) come out in
    a different order every run, the results computed from them do not (tests/test_gpu_graphs.py: detections bit for bit)."""

    def __init__(self, model, cfg, device, depth=None):
        from . import GRAPH_REPLAY_SAFE
        if not GRAPH_REPLAY_SAFE:
            raise RuntimeError("GraphedRunner: DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was not in place when the HIP runtime started "
                               "(see the package's __init__): replaying graphs is unsafe on this runtime; use make_runner()")
        super().__init__(model, cfg, device, depth)
        have = _RUNNER_STREAMS[(str(self.device), 0)]
        # the feature-stream graphs are CAPTURED on a stream of their own (a capture cannot run on the default stream) and REPLAYED on
        # the caller's stream, as PipelinedRunner runs them: a fifth busy stream would share one of the four hardware queues with
        # another one and serialise behind it (measured: 4155 instead of 5470 scenes/s at K = 100).  The C library's scratch of the
        # capture stream is theirs alone -- every one of these graphs replays on the same stream, in order.
        if have.get("feat") is None:
            have["feat"] = torch.cuda.Stream(self.device)
        self.feat = have["feat"]
        # depth / group groups ahead + the one being consumed.  One more (the first version) costs 5.5 % at K = 96 -- 5100-5160 instead of
        # 5406 scenes/s, the eager runner's figure: a fifth of the slots' 23 GB more to walk through per rotation; one less stalls (2765)
        # never fewer than 2: the slot of the batch in flight must not be the one the next chain is written into
        want = int(os.environ.get("PRCNN_GRAPH_SLOTS", "0"))
        if want == 1 or want < 0:
            raise ValueError("PRCNN_GRAPH_SLOTS=%d: the graphed runner needs at least 2 group slots" % want)
        self.n_slots = want or max(2, -(-self.depth // self.group) + 1)
        # PAIR consecutive batches of a group share the launches of every stage behind the geometry (RPN stage, proposal layer + RoI
        # geometry, RCNN features, final stage): one MEMBER of a slot = `pair` batches = pair x B scenes per launch.  Fatter launches:
        # the same 160 / 800 scenes run 4 % / 3.5 % faster in steps of 16 than in steps of 8; the detections of a
        # batch come back up to 2 pair - 1 submits late instead of 1.
        self.pair = max(1, RCNN_PAIR)
        if self.group % self.pair:
            self.pair = 1
        self.shape = None
        self._assigned = []          # [(batch tensor, group slot, batch index within the slot)] chains launched, batch not yet submitted
        self._pending = None         # the member being filled: {"s": slot, "m": member, "halves": set of batch positions submitted so far}
        self._inflights = collections.deque()    # ("graph", slot, member, [valid batch positions]) | ("eager", det), oldest first
        self._out = collections.deque()          # detections finished and not handed back yet, in submit order
        self._next_slot = 0
        self._max_todo = 0           # the longest look-ahead a submit() has seen
        self.captures = 0

    # ---- capture -------------------------------------------------------------------------------------------------------------
    def _capture(self, stream, pool, fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            stream.synchronize()
            # thread_local: other threads of the process (pinned-memory loaders, writers) may call into HIP during a capture
            g.capture_begin(pool=pool, capture_error_mode="thread_local")
            try:
                out = fn()
            finally:
                g.capture_end()
        self.captures += 1
        return g, out

    @torch.no_grad()
    def _build(self, first):
        """slots, warm-up of every role stream (the C library's per-stream scratch must exist before a capture), the captures"""
        eng, cfg, G = self.engine, self.cfg, self.group
        B, N, _ = first.shape
        self.shape = tuple(first.shape)
        P = self.pair
        Bm, Gm = P * B, G // P                                   # scenes per member launch, members per slot
        eng.check_weights()
        torch.cuda.synchronize(self.device)
        self.xin = [torch.empty((G * B, N, 3), dtype=torch.float32, device=self.device) for _ in range(self.n_slots)]
        for x in self.xin:
            for k in range(G):
                x[k * B:(k + 1) * B].copy_(first)              # valid clouds everywhere: a partly filled group computes on them
        parts = lambda s: [self.xin[s][k * Bm:(k + 1) * Bm] for k in range(Gm)]

        def tail_stage(st):
            rois, roi_scores = eng.propose(st)
            return {"rois": rois, "roi_scores": roi_scores, "rg": eng.rcnn_geometry(st, rois)}

        def final_stage(tl, out):
            ret = {"rois": tl["rois"], "rcnn_cls": out["rcnn_cls"], "rcnn_reg": out["rcnn_reg"]}
            det = postprocess(cfg, ret, Bm, blob_scenes=B if P > 1 else None)
            det.update(ret)
            return det

        # warm-up, eagerly, once per stream that will capture (and to have real data behind every pointer while capturing)
        for side in self.sides:
            with torch.cuda.stream(side):
                geos = eng.geometry_group(parts(0))
            side.synchronize()
        with torch.cuda.stream(self.feat):
            st = eng.rpn_stage(parts(0)[0], geos[0])
        self.feat.synchronize()
        with torch.cuda.stream(self.tail):
            tl = tail_stage(st)
        self.tail.synchronize()
        with torch.cuda.stream(self.feat):
            out = eng.rcnn_features(tl["rg"])
        self.feat.synchronize()
        with torch.cuda.stream(self.tail):
            final_stage(tl, out)
        self.tail.synchronize()
        del geos, st, tl, out

        # ONE MEMORY POOL PER GRAPH.  Graphs that share a pool may only be replayed in the order of their capture with the outputs of
        # the later ones dead: the temporaries of an earlier capture are free memory when the later one allocates its OUTPUTS, so
        # replaying the earlier graph writes over them (seen: the geometry graph of slot 0 replayed while the RPN stages of slot 4
        # still needed slot 4's index tables -> memory fault).  The slots rotate, so no such order exists here.
        mem0 = torch.cuda.memory_reserved(self.device)
        pool = torch.cuda.graph_pool_handle
        self.slots = []
        for s in range(self.n_slots):
            side = self.sides[s % len(self.sides)]
            g_geo, geos = self._capture(side, pool(), lambda: eng.geometry_group(parts(s)))
            slot = {"side": side, "g_geo": g_geo, "geos": geos, "ev_geo": torch.cuda.Event(), "members": []}
            for k in range(Gm):
                xb = parts(s)[k]
                g_rpn, st = self._capture(self.feat, pool(), lambda: eng.rpn_stage(xb, geos[k]))
                g_tail, tl = self._capture(self.tail, pool(), lambda: tail_stage(st))
                g_rcnn, out = self._capture(self.feat, pool(), lambda: eng.rcnn_features(tl["rg"]))
                # (captured on the stream family it replays on: its kernels' library scratch is keyed by the capture stream, and graphs
                #  that share scratch must replay on one stream, in order)
                g_post, det = self._capture(self.tail, pool(), lambda: final_stage(tl, out))
                slot["members"].append({"g_rpn": g_rpn, "g_tail": g_tail, "g_rcnn": g_rcnn, "g_post": g_post,
                                        "st": st, "tl": tl, "out": out, "det": det,
                                        "ev_rpn": torch.cuda.Event(), "ev_prop": torch.cuda.Event(), "ev_rcnn": torch.cuda.Event(),
                                        "ready": torch.cuda.Event(), "used": False})
            self.slots.append(slot)
        self.graph_bytes = torch.cuda.memory_reserved(self.device) - mem0
        torch.cuda.synchronize(self.device)

    def _conforms(self, pts):
        return (pts is not None and pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 3 and pts.shape[-1] == 3 and
                (self.shape is None or tuple(pts.shape) == self.shape))

    # ---- replay --------------------------------------------------------------------------------------------------------------
    def _debug(self, bit, message, *args):
        """PRCNN_GRAPH_DEBUG (bit mask; 1: before a geometry graph, 2: after it, 4: after every stage of a member): device sync + print"""
        if _GRAPH_DEBUG & bit:
            torch.cuda.synchronize(self.device)
            print("[graph debug] " + message % args, flush=True)

    def _where(self, pts):
        for a in self._assigned:
            if a[0] is pts:
                return a
        return None

    def _target_slot_state(self):
        """the slot the next chain would be written into -> (slot index, holds a batch in flight or the member being filled?, holds
        assigned batches that were not submitted yet?)"""
        s = self._next_slot % self.n_slots
        busy = any(f[0] == "graph" and f[1] == s for f in self._inflights) or (self._pending is not None and self._pending["s"] == s)
        return s, busy, any(a[1] == s for a in self._assigned)

    def _launch_group(self, batch_list, main):
        s = self._next_slot % self.n_slots
        self._next_slot += 1
        slot = self.slots[s]
        side = slot["side"]
        B = self.shape[0]
        side.wait_stream(main)                              # the batches are ready on the caller's stream
        for m in slot["members"]:
            if m["used"]:
                side.wait_event(m["ev_rcnn"])               # the slot's previous batches have been read to the end
                m["used"] = False
        with torch.cuda.stream(side):
            for k, pts in enumerate(batch_list):
                self.xin[s][k * B:(k + 1) * B].copy_(pts, non_blocking=True)
            self._debug(1, "geometry of slot %d: %d batches", s, len(batch_list))
            slot["g_geo"].replay()
            slot["ev_geo"].record(side)
            self._debug(2, "geometry of slot %d done", s)
        for k, pts in enumerate(batch_list):
            self._assigned.append((pts, s, k))

    @torch.no_grad()
    def submit(self, cur, upcoming=None):
        """-> the detections of an EARLIER batch (in submit order), or None"""
        main = torch.cuda.current_stream(self.device)
        todo = self._look_ahead(upcoming)
        if self.shape is None and self._conforms(cur):
            self._build(cur)
        if not self._conforms(cur) or self.shape is None:
            return self._submit_eager(cur, main)
        todo = [p for p in todo if self._conforms(p)]
        a = self._where(cur)
        if a is None:                                       # cold start (or a caller that looks less far ahead)
            self.engine.check_weights()
            self._close_pending(main)                       # a member left half filled: its batches run now
            s_next, busy, holds_assigned = self._target_slot_state()
            if busy:                                        # few slots: a batch in flight lives where this chain goes -- its RCNN and
                self._finish_slot(s_next)                   # final stages are enqueued first (the chain waits for ev_rcnn)
            if holds_assigned:                              # batches announced earlier and never submitted: their chain is dropped
                self._assigned[:] = [x for x in self._assigned if x[1] != s_next]
            self._launch_group([cur] + [p for p in todo if self._where(p) is None][:self.group - 1], main)
            a = self._where(cur)
        self._assigned[:] = [x for x in self._assigned if x is not a]
        missing = [p for p in todo if self._where(p) is None]
        # a look-ahead that got SHORTER than the caller's usual one: the run is ending and `missing` is all that is left -- its chain
        # starts now, not when the pipeline is about to run dry (the last, partly filled group of a run whose length is not a multiple
        # of the group used to be launched 1-2 steps before its first batch was due: a 3 ms chain, 2 ms of stall; K = 30: 5830 -> 6400)
        self._max_todo = max(self._max_todo, len(todo))
        if self._next_group_due(todo, missing, ending=len(todo) < self._max_todo):
            s_next, busy, holds_assigned = self._target_slot_state()
            # a look-ahead chain is optional: it waits for a later submit while its slot still holds the current batch or batches
            # that were assigned and not submitted yet; the slot of a batch in flight is released by finishing that batch first
            pend_here = self._pending is not None and self._pending["s"] == s_next
            if not holds_assigned and s_next != a[1] and not pend_here:
                if busy:
                    self._finish_slot(s_next)
                self.engine.check_weights()
                self._launch_group(missing[:self.group], main)
        _, s, k = a
        m, h = k // self.pair, k % self.pair
        if self._pending is not None and (self._pending["s"], self._pending["m"]) != (s, m):
            self._close_pending(main)                       # the caller skipped the rest of that member
        if self._pending is None:
            self._pending = {"s": s, "m": m, "halves": set()}
        self._pending["halves"].add(h)
        if h == self.pair - 1:
            self._close_pending(main)
        return self._out.popleft() if self._out else None

    def _close_pending(self, main):
        """RPN stage and proposal stage of the member being filled (its batches not submitted hold an earlier pass's clouds: computed,
        never handed back), then the RCNN + final stages of the member in flight behind them"""
        p, self._pending = self._pending, None
        if p is None:
            return
        s, mi = p["s"], p["m"]
        slot = self.slots[s]
        m = slot["members"][mi]
        feat, tail = main, self.tail
        feat.wait_event(slot["ev_geo"])
        with torch.cuda.stream(feat):
            m["g_rpn"].replay()
            m["ev_rpn"].record(feat)
        self._debug(4, "slot %d member %d rpn done", s, mi)
        tail.wait_event(m["ev_rpn"])
        with torch.cuda.stream(tail):
            m["g_tail"].replay()
            m["ev_prop"].record(tail)
        self._debug(4, "slot %d member %d tail done", s, mi)
        if self._inflights:
            self._finish_inflight()
        m["used"] = True
        self._inflights.append(("graph", s, mi, sorted(p["halves"])))

    def _submit_eager(self, cur, main):
        self._close_pending(main)
        while self._inflights:                              # another shape: the pipeline drains first (results stay in order)
            self._finish_inflight()
        det = infer_batch(self.model, self.cfg, cur, engine=self.engine)
        ready = torch.cuda.Event()
        ready.record(main)
        det["ready"], det["stream"] = ready, main
        self._inflights.append(("eager", det))
        return self._out.popleft() if self._out else None

    def _finish_slot(self, s):
        """RCNN + final stages of every batch in flight up to the last one that lives in group slot `s` (in order)"""
        if self._pending is not None and self._pending["s"] == s:
            self._close_pending(torch.cuda.current_stream(self.device))
        while any(f[0] == "graph" and f[1] == s for f in self._inflights):
            self._finish_inflight()

    def _finish_inflight(self):
        """RCNN + final stages of the OLDEST member in flight; its batches' detections go onto self._out"""
        if not self._inflights:
            return
        f = self._inflights.popleft()
        if f[0] == "eager":
            self._out.append(f[1])
            return
        _, s, mi, halves = f
        m = self.slots[s]["members"][mi]
        feat, tail = torch.cuda.current_stream(self.device), self.tail
        feat.wait_event(m["ev_prop"])
        with torch.cuda.stream(feat):
            m["g_rcnn"].replay()
            m["ev_rcnn"].record(feat)
        self._debug(4, "slot %d member %d rcnn done", s, mi)
        tail.wait_event(m["ev_rcnn"])
        with torch.cuda.stream(tail):
            m["g_post"].replay()
            m["ready"].record(tail)
        self._debug(4, "slot %d member %d done", s, mi)
        if self.pair == 1:
            det = dict(m["det"])
            det["ready"], det["stream"] = m["ready"], tail
            self._out.append(det)
            return
        B = self.shape[0]
        for h in halves:                                    # one detections dict per batch: views of the member's tensors
            det = {}
            blobs = m["det"].get("blobs")
            for key, v in m["det"].items():
                if key in ("blob", "blobs"):
                    continue
                if isinstance(v, list):                     # per-batch views of the batch's own blob (boxes, scores, num)
                    det[key] = v[h]
                elif torch.is_tensor(v):
                    per = v.shape[0] // self.pair           # rows of this tensor per batch (B scenes, or B x rois)
                    det[key] = v[h * per:(h + 1) * per]
            # round 5: the final stage writes one blob per BATCH of the member (prcnn_rcnn_postprocess_blobs): one copy per batch
            det["blob"] = blobs[h] if blobs is not None else None
            det["ready"], det["stream"] = m["ready"], tail
            self._out.append(det)

    @torch.no_grad()
    def flush(self):
        """Finish what is still in the pipeline and return the detections of the OLDEST batch not handed back yet; None when nothing is
        left (call until then: with pair = 2 up to three batches are outstanding).  Chains of batches never submitted are dropped."""
        self._assigned[:] = []
        if not self._out:
            self._close_pending(torch.cuda.current_stream(self.device))
            while self._inflights and not self._out:
                self._finish_inflight()
        return self._out.popleft() if self._out else None

    @torch.no_grad()
    def reload_weights(self):
        """The model's weights were changed on purpose (the next checkpoint of a sweep): FastPointRCNN.reload_weights() writes through
        the addresses the captured graphs replay, ordered against the side and tail streams -- NO graph is captured again
        (`captures` stays what it was).  RuntimeError while a batch is in flight or has not been handed back -- flush() until None
        first.  Chains of batches that were announced and not submitted are dropped, as flush() drops them."""
        if self._pending is not None or self._inflights or self._out:
            raise RuntimeError("GraphedRunner.reload_weights: a batch is in flight; flush() until it returns None first")
        self._assigned[:] = []
        self._reload_ordered()

    def _role_streams(self):
        return [self.tail, self.feat] + list(self.sides)


def _tensors(obj):
    if torch.is_tensor(obj):
        if obj.device.type != "meta":             # (a shape-only index tensor: dropin/pointnet2_cuda.py rcnn_roi_geometry_packs_wrapper)
            yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)
    elif hasattr(obj, "rowinfo"):                 # BallPack (distinct-row list of an index tensor)
        for v in obj.tensors():
            yield v
