"""Joint RPN+RCNN evaluation harness: the counterpart of the hot loop of
pointrcnn/tools/eval_rcnn.py (eval_one_epoch_joint :466-690, save_kitti_format :76-101,
checkpoint loading via train_utils.load_checkpoint :78-92) for synthetic KITTI-shaped scenes.

Differences that are deliberate:
  * the per-scene tail (score threshold -> sort -> rotated NMS -> D2H, :611-635) is batched on
    the device: one masked sort, one launch of the device-resident NMS for all scenes, ONE D2H
    copy per batch of fixed-shape (B,M,7)/(B,M)/(B) tensors;
  * scenes shard across ranks (rank r takes scenes r, r+W, ...) and detections are combined with
    one all_gather at the end (the reference is single-process);
  * the reference's dataloader bug (`far_points=` keyword, eval_rcnn.py:862) is not reproduced.

CLI (subset of the reference's flags):  python -m ... --cfg_file X --eval_mode rcnn --ckpt Y [--rpn_ckpt C] [--rcnn_ckpt C]
  --batch_size 8 --output_dir out [--set K V ...] [--scenes 64]
  --eval_all --ckpt_dir D [--start_epoch E] [--extra_tag T] [--wait SECONDS]: every unevaluated checkpoint of D (eval_sweep.py)
"""
import argparse
import collections
import contextlib
import os
import time

import numpy as np
import torch

from . import config as config_mod
from .net.point_rcnn import PointRCNN
# every name below is part of this module's surface (bench.py, the tests and profiles/ read them here); code that PATCHES one of them
# has to patch the module that defines and reads it
from .runners import (_RUNNER_STREAMS, _runner_streams, PipelinedRunner, ModuleRunner, EngineRunner, RpnRunner, GraphedRunner,
                      make_runner, engine_covers, native_modules, reference_api_only, USE_GRAPHS, RCNN_PAIR, _GRAPH_DEBUG, _tensors,
                      _anchor_host, _anchor_on, split_detections, postprocess, infer_batch, FUSED_POSTPROCESS, FastPointRCNN)
from .host import (_NODE_AFFINITY, _node_affinity, _cpu_topology, slice_topology, host_budget, pin_to_budget, PIN_CORES,
                   _limit_worker_threads)
from .gather import shard_scene_ids, pack_detections, all_gather_detections
from .results import (kitti_result_text, kitti_result_lines, save_kitti_format, detections_to_annos, evaluate_detections, prepare_gt, RecallStats,
                      _calib_row, _RowCalib, _write_batch, _write_rpn_batch)



def build_model(cfg, device, seed=0):
    """Random-init PointRCNN in TEST mode (eval_rcnn.py:758), deterministic in ``seed``."""
    torch.manual_seed(seed)
    model = PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TEST")
    return model.to(device).eval()


def load_checkpoint(model, filename, logger=None):
    """Accepts the reference's .pth layout {'model_state','optimizer_state','epoch','it'}
    (train_utils.py:60-92); also a bare state_dict."""
    ckpt = torch.load(filename, map_location="cpu")
    state = ckpt["model_state"] if isinstance(ckpt, dict) and "model_state" in ckpt else ckpt
    model.load_state_dict(state)
    return ckpt.get("epoch", -1) if isinstance(ckpt, dict) else -1


LOADER_TARGET = 6500.0          # scenes/s the loader processes are sized for


def _shm_worker(source, scene_ids, batch_size, raw, buf, tasks, results, pin=None):
    """A loader process of _ShmFeed: takes (batch index, slot), produces the batch's scenes STRAIGHT INTO the slot of the shared,
    pinned buffer -- sampled clouds (B, npoints, c) or, for the device input stage, raw clouds packed (B, n_max, stride) -- and sends
    back only the small things: per-scene counts, calibration rows, image shapes."""
    _limit_worker_threads()
    if pin:                     # (a fork server that was started before the parent confined itself hands out its own, wider affinity)
        try:
            os.sched_setaffinity(0, pin)
        except (AttributeError, OSError):
            pass
    flat = buf.numpy()
    try:
        while True:
            t = tasks.get()
            if t is None:
                return
            b, slot = t
            ids = scene_ids[b * batch_size:(b + 1) * batch_size]
            loaded = [source.load_raw(i) if raw else source.load(i) for i in ids]
            arrs = [np.ascontiguousarray(l[0], dtype=np.float32) for l in loaded]
            n_max, c = max(1, max(a.shape[0] for a in arrs)), arrs[0].shape[1]
            if len(ids) * n_max * c > flat.shape[1]:
                raise RuntimeError("a batch of %d clouds x %d points x %d floats does not fit a loader slot of %d floats "
                                   "(PRCNN_RAW_SLOT_POINTS)" % (len(ids), n_max, c, flat.shape[1]))
            dst = flat[slot, :len(ids) * n_max * c].reshape(len(ids), n_max, c)
            for k, a in enumerate(arrs):
                dst[k, :a.shape[0]] = a                           # (rows beyond a raw cloud's length are never read: counts)
            results.put((b, slot, n_max, c, [a.shape[0] for a in arrs], np.stack([_calib_row(l[1]) for l in loaded], 0),
                         [tuple(l[2]) for l in loaded]))
    except BaseException as e:                                      # noqa: BLE001 -- the parent re-raises it
        import traceback
        results.put((-1, -1, 0, 0, "loader process failed: %r\n%s" % (e, traceback.format_exc()), None, None))


class _ShmFeed:
    """Loader processes that write into ONE shared, page-locked buffer (round 6).  torch's DataLoader hands every
    batch (device input stage: every raw cloud) over as a tensor in a shared-memory file of its own -- a file descriptor through a unix
    socket per tensor, a copy into pinned memory by a thread of the parent, then the upload: 2.4 ms of the feeding thread per batch of raw
    clouds (profiles/r06_driver.md), the whole driver at 2400 scenes/s beside an engine that does 6500.  Here the buffer is allocated once
    (torch shared memory), registered with the HIP runtime (hipHostRegister: uploads from it are asynchronous DMA), cut into slots, and a
    loader fills the slot its task names; the parent receives a dozen integers and 33 floats per scene, views the slot and enqueues the
    upload.  A slot returns to the free list when its upload has completed (an event).  Batches come back in order."""

    def __init__(self, source, scene_ids, batch_size, raw, workers, ctx, pin, slot_floats, cpus=None):
        import torch.multiprocessing as tmp
        self.batch_size, self.raw = batch_size, raw
        self.n_batches = -(-len(scene_ids) // batch_size)
        n_slots = min(self.n_batches, 2 * workers + 4)
        self.buf = torch.empty((n_slots, slot_floats), dtype=torch.float32).share_memory_()
        self.registered = False
        if pin:
            rc = torch.cuda.cudart().cudaHostRegister(self.buf.data_ptr(), self.buf.numel() * 4, 0)
            self.registered = int(rc) == 0
        mp = tmp.get_context(ctx)
        self.tasks, self.results = mp.Queue(), mp.Queue()
        self.procs = [mp.Process(target=_shm_worker, args=(source, list(scene_ids), batch_size, raw, self.buf, self.tasks, self.results, cpus), daemon=True)
                      for _ in range(workers)]
        for p in self.procs:
            p.start()
        self.free, self.busy, self.ready = collections.deque(range(n_slots)), collections.deque(), {}
        self.next_task = self.next_out = 0
        self._feed()

    def _feed(self):
        while self.busy and self.busy[0][1].query():
            self.free.append(self.busy.popleft()[0])
        while self.free and self.next_task < self.n_batches:
            self.tasks.put((self.next_task, self.free.popleft()))
            self.next_task += 1

    def next(self):
        """-> (host tensor (B, n_max, c): a view of the slot, slot, counts, calibs, shapes) of the next batch, or None at the end"""
        if self.next_out >= self.n_batches:
            return None
        while self.next_out not in self.ready:
            if not self.free and self.next_task < self.n_batches and self.busy and len(self.ready) == 0 and self.results.empty():
                self.busy[0][1].synchronize()                     # every slot is waiting for its upload: wait for the oldest one
                self._feed()
            try:
                r = self.results.get(timeout=1.0)
            except Exception:                                      # noqa: BLE001 (queue.Empty): keep the workers fed, notice dead ones
                self._feed()
                dead = [p.exitcode for p in self.procs if p.exitcode not in (None, 0)]
                if dead or not any(p.is_alive() for p in self.procs):
                    raise RuntimeError("eval_scenes: a loader process has exited (exit codes %s): its batch will never arrive" % (dead or "0"))
                continue
            if r[0] < 0:
                raise RuntimeError(r[4])
            self.ready[r[0]] = r[1:]
        slot, n_max, c, counts, rows, shapes = self.ready.pop(self.next_out)
        self.next_out += 1
        host = self.buf[slot, :len(counts) * n_max * c].view(len(counts), n_max, c)
        return host, slot, counts, [_RowCalib(rows[k]) for k in range(len(counts))], shapes

    def release(self, slot, event):
        """the slot's upload has been enqueued behind `event` (None: the data has been consumed already)"""
        if event is None:
            self.free.append(slot)
        else:
            self.busy.append((slot, event))
        self._feed()

    def close(self):
        for _ in self.procs:
            self.tasks.put(None)
        for p in self.procs:
            p.join(timeout=5)
            if p.is_alive():
                p.terminate()
        if self.registered:
            torch.cuda.synchronize()
            torch.cuda.cudart().cudaHostUnregister(self.buf.data_ptr())
            self.registered = False


def eval_scenes(*args, **kwargs):
    """eval_scenes_pinned with the process's CPU affinity put back afterwards (the driver confines itself and its loader / writer
    processes to the rank's cores: host_budget / pin_to_budget; a caller that goes on to other work -- bench.py's CPU baseline --
    gets the whole host back)."""
    try:
        before = os.sched_getaffinity(0)
    except (AttributeError, OSError):
        before = None
    try:
        return eval_scenes_pinned(*args, **kwargs)
    finally:
        if before is not None:
            # EVERY thread of the process: sched_setaffinity(0) moves the calling thread only, and pool threads (OpenMP, BLAS) that
            # were created while the driver was confined inherited its 32 cores -- bench.py's CPU baseline, which runs afterwards
            # on 128 threads, took 138 s instead of 27 behind a driver leg that had restored the main thread alone
            try:
                tids = [int(t) for t in os.listdir("/proc/self/task")]
            except OSError:
                tids = [0]
            for tid in tids:
                try:
                    os.sched_setaffinity(tid, before)
                except OSError:
                    pass


@torch.no_grad()
def eval_scenes_pinned(model, cfg, device, source, scene_ids, batch_size=8, output_dir=None, workers=None, device_input=False,
                       recall=None, stats=None, runner=None):
    """Evaluate ``scene_ids`` of a scene source (kitti_io.KittiSource / SyntheticSource) on this rank:
    the counterpart of the batch loop of eval_one_epoch_joint (eval_rcnn.py:493-649) incl. the KITTI
    result files.  Returns (table, counts) as pack_detections.

    ``workers`` loader processes read / filter / subsample scenes ahead of the device (the reference's
    DataLoader workers, eval_rcnn.py:868-871): a scene costs milliseconds of numpy on the host, the device
    needs ~1.3 ms per scene, so a single-threaded loader would be the bottleneck.  Batches arrive in order.
    ``device_input``: the loaders only READ the raw clouds (``source.load_raw``); rectification, validity filter
    and the near/far sampler run on the device (kitti_io.DeviceInputStage, csrc/input_stage.hip).
    ``recall``: a RecallStats that receives every batch's RoIs / refined boxes and the source's ground-truth boxes
    (the reference's recall statistics, skipped with --test).  ``stats``: a dict that receives the completion time of
    every batch (``batch_done``), for steady-state throughput measurements.  ``runner``: a runner of ``model`` that the caller
    keeps across calls (the checkpoint sweep: its engine and captured graphs stay, the weights are reloaded in between); it comes
    back flushed."""
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
    M = cfg.TEST.RPN_POST_NMS_TOP_N
    on_gpu = torch.device(device).type == "cuda"
    if runner is None:
        runner = make_runner(model, cfg, device) if on_gpu else None
    budget = host_budget()
    if stats is not None:
        stats["host_budget"] = {"loaders": budget["loaders"], "writers": budget["writers"], "cores": len(budget["cores"]), "pin": len(budget["pin"]),
                                "pinned": pin_to_budget(budget)}
    else:
        pin_to_budget(budget)
    starts = list(range(0, len(scene_ids), batch_size))
    if workers is None:
        workers = budget["loaders"]
        if "PRCNN_LOADER_WORKERS" not in os.environ and len(starts) > 2:
            # as many loaders as THIS source needs to feed the engine: a scene is timed here, in the parent (the uniform generator costs
            # ~0.8 ms, the KITTI reader + sampler of kitti_io.KittiSource ~2 ms, a raw .bin read 0.3 ms), and the count covers
            # LOADER_TARGET scenes/s with a third to spare -- at least the budget's 6, at most 12, inside the rank's share of the host.  More is NOT better
            # (profiles/r06_driver_sweep.md, KITTI tree + host sampler: 6 loaders 4060, 12: 5200-5650, 18: 4900, 24: 4700 scenes/s, and
            # 4 writers instead of 2 cost another 15 %; round 5 found the same for the uniform source): every runnable process
            # beyond what the engine consumes takes clock and memory bandwidth from the one thread that feeds the GPU
            load_one = source.load_raw if device_input else source.load
            load_one(scene_ids[0])                                  # (first touch: imports, page cache)
            t0 = time.perf_counter()
            load_one(scene_ids[min(1, len(scene_ids) - 1)])
            t_load = time.perf_counter() - t0
            spare = max(1, len(budget.get("pin") or budget["cores"]) - 1 - budget["writers"])
            workers = int(max(min(workers, spare), min(np.ceil(t_load * LOADER_TARGET * 1.33), 12, spare)))
            if stats is not None:
                stats["loader_calibration"] = {"ms_per_scene": round(t_load * 1e3, 2), "loaders": workers}
    stage = None
    if device_input:
        if not on_gpu:
            raise RuntimeError("eval_scenes: device_input needs a GPU")
        from . import kitti_io
        stage = kitti_io.DeviceInputStage(cfg, device, npoints_faraway=getattr(source, "npoints_faraway", 4000),
                                          seed=getattr(source, "seed", 1024))
    feed = None
    if workers > 0 and len(starts) > 2:
        # loader PROCESSES (the scene generator / KITTI reader is Python + numpy: threads would serialise on the GIL) that write into
        # one shared page-locked buffer (_ShmFeed); the parent views a slot and enqueues its upload.
        # Forking a process whose HIP runtime is already initialised is unsupported (sporadic hangs at worker start or
        # exit): once the GPU has been touched the workers come from a fork SERVER (clean interpreters, picklable dataset).
        ctx = "forkserver" if (on_gpu and torch.cuda.is_initialized()) else "fork"
        ctx = os.environ.get("PRCNN_LOADER_CONTEXT", ctx)
        if stage is not None:
            slot_floats = batch_size * int(os.environ.get("PRCNN_RAW_SLOT_POINTS", "200000")) * 4
        else:
            slot_floats = batch_size * cfg.RPN.NUM_POINTS * (4 if cfg.RPN.USE_INTENSITY else 3)
        feed = _ShmFeed(source, scene_ids, batch_size, stage is not None, workers, ctx, on_gpu, slot_floats,
                        cpus=None if os.environ.get("PRCNN_NO_AFFINITY") == "1" else list(budget.get("pin") or budget["cores"]))
        if stats is not None:
            stats["loader_buffer"] = {"slots": int(feed.buf.shape[0]), "MB": round(feed.buf.numel() * 4 / 1e6, 1), "page_locked": feed.registered}

    writers = None
    try:                                   # (the loader processes, their page-locked buffer and the writer pool are released on every way out)
        feed_wait = [0.0]                      # seconds the feeding thread spent inside feed.next() (waiting for a loader + unpacking its message)

        def load(s):
            ids = scene_ids[s:s + batch_size]
            if not ids:
                return None, ids, None
            if feed is not None:
                tw = time.perf_counter()
                host, slot, counts, calibs, shapes = feed.next()
                feed_wait[0] += time.perf_counter() - tw
                meta = list(zip(calibs, shapes))
                if stage is not None:
                    pts, _ = stage.from_packed(host, counts, calibs, shapes, ids, lidar_frame=source.raw_in_lidar_frame,
                                               image_filter=source.raw_needs_image_filter)
                    feed.release(slot, stage.last_done)
                    return pts, ids, meta
                if not on_gpu:
                    pts = host.clone()
                    feed.release(slot, None)
                    return pts, ids, meta
                if feed.registered:
                    pts = host.to(device, non_blocking=True)
                else:                                                   # registration refused: through a pinned staging copy
                    pts = host.pin_memory().to(device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
                feed.release(slot, ev)
                return pts, ids, meta
            if stage is not None:
                raws = [source.load_raw(i)[0] for i in ids]
                meta = [source.calib_and_shape(i) for i in ids]
                pts, _ = stage(raws, [m[0] for m in meta], [m[1] for m in meta], ids,
                               lidar_frame=source.raw_in_lidar_frame, image_filter=source.raw_needs_image_filter)
                return pts, ids, meta
            loaded = [source.load(i) for i in ids]
            host = torch.from_numpy(np.stack([l[0] for l in loaded], 0))
            host = host.pin_memory() if on_gpu else host
            meta = [(l[1], l[2]) for l in loaded]
            return host.to(device, non_blocking=True), ids, meta

        # Results are consumed LATE: the D2H copy of a batch is queued (on the stream that produced it) the moment the batch
        # is submitted, but the host only waits for it `lag` batches later, when it has long completed -- the host thread
        # never stalls on the GPU inside the loop and keeps enqueueing ahead of it.  The KITTI text files are written by a
        # small thread pool (numpy projection + formatting + file I/O per scene; the reference does this inline, :635).
        import collections
        from concurrent.futures import ProcessPoolExecutor
        import multiprocessing
        lag = int(os.environ.get("PRCNN_RESULT_LAG", "3")) if runner is not None else 0
        inflight = collections.deque()
        # writer PROCESSES: the formatting of ~40 text lines per scene is pure Python and would hold the GIL of the thread
        # that feeds the GPU; one job per batch
        writers = None
        if output_dir:
            wctx = "forkserver" if (on_gpu and torch.cuda.is_initialized()) else "fork"
            writers = ProcessPoolExecutor(max_workers=budget["writers"], initializer=_limit_worker_threads,
                                          mp_context=multiprocessing.get_context(os.environ.get("PRCNN_LOADER_CONTEXT", wctx)))
        jobs = []
        results = {}

        def start_copy(det, ids, meta, order):
            with torch.cuda.stream(det["stream"]) if "stream" in det else contextlib.nullcontext():
                if on_gpu and det.get("blob") is not None:
                    hb = torch.empty(det["blob"].shape, dtype=torch.float32, pin_memory=True)
                    hb.copy_(det["blob"], non_blocking=True)            # boxes | scores | num in one transfer
                    host = list(split_detections(hb, det["boxes"].shape[0], det["boxes"].shape[1]))
                    done = torch.cuda.Event()
                    done.record()
                elif on_gpu:
                    host = [torch.empty(det[k].shape, dtype=det[k].dtype, pin_memory=True) for k in ("boxes", "scores", "num")]
                    for h, k in zip(host, ("boxes", "scores", "num")):
                        h.copy_(det[k], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record()
                else:
                    host, done = [det[k] for k in ("boxes", "scores", "num")], None
                if recall is not None:
                    recall.update(det["pred_boxes3d"], det["rois"], [source.gt_boxes3d(i) for i in ids])
            inflight.append((host, done, ids, meta, order))

        def consume():
            (boxes, scores, num), done, ids, meta, order = inflight.popleft()
            if done is not None:
                done.synchronize()
            results[order] = (boxes, scores, num)
            if stats is not None:
                stats.setdefault("batch_done", []).append(time.perf_counter())
            if output_dir:
                nn = num.tolist()
                jobs.append(writers.submit(_write_batch, ids, [m[0] for m in meta], [m[1] for m in meta],
                                           [boxes[k, :nn[k]].numpy() for k in range(len(ids))],
                                           [scores[k, :nn[k]].numpy() for k in range(len(ids))], output_dir, cfg.CLASSES))

        # software pipeline: while batch i is on the device, batch i+1 is loaded and (three-stream runner) the RCNN +
        # final stage of batch i-1 complete; results are consumed `lag` batches late
        submitted = collections.deque()        # (ids, meta, order) of the batches whose detections have not come back yet, oldest first
        order = 0
        depth = runner.depth if runner is not None else 1
        ahead = [load(k * batch_size) for k in range(depth)]   # `depth` batches ahead: the runner starts their geometry chains early
        phase = {"load": 0.0, "submit": 0.0, "copy": 0.0, "consume": 0.0} if stats is not None else None     # host seconds of the feeding thread by phase
        clock = time.perf_counter
        for s in range(0, len(scene_ids), batch_size):
            pts, ids, meta = ahead.pop(0)
            t0, w0 = clock(), feed_wait[0]
            ahead.append(load(s + depth * batch_size))
            t1 = clock()
            if runner is not None:
                det = runner.submit(pts, [a[0] for a in ahead])        # an earlier batch's detections (in submit order), or None
                submitted.append((ids, meta, order))
                t2 = clock()
                if det is not None:
                    start_copy(det, *submitted.popleft())
            else:
                t2 = clock()
                start_copy(infer_batch(model, cfg, pts), ids, meta, order)
            t3 = clock()
            order += 1
            while len(inflight) > lag:
                consume()
            if phase is not None and order > depth:                    # (steady state: behind the first look-ahead's worth of batches)
                phase["feed_next"] = phase.get("feed_next", 0.0) + feed_wait[0] - w0
                phase["load"] += t1 - t0 - (feed_wait[0] - w0); phase["submit"] += t2 - t1; phase["copy"] += t3 - t2; phase["consume"] += clock() - t3
                phase["batches"] = phase.get("batches", 0) + 1
        if phase is not None:
            stats["host_phases_ms_per_batch"] = {k: round(v / max(1, phase.get("batches", 1)) * 1e3, 3) for k, v in phase.items() if k != "batches"}
        while runner is not None and submitted:
            det = runner.flush()                                        # one batch per call, oldest first
            if det is None:
                raise RuntimeError("eval_scenes: the runner returned no detections for %d submitted batches" % len(submitted))
            start_copy(det, *submitted.popleft())
        while inflight:
            consume()
        for j in jobs:
            j.result()
    finally:
        if writers is not None:
            writers.shutdown(wait=True, cancel_futures=True)
        if feed is not None:
            feed.close()
    return pack_detections(scene_ids, [results[k] for k in sorted(results)], M)


def steady_state_rate(stats, batch_size):
    """scenes/s between the completion of the first and of the last batch (loader / writer process start-up excluded)"""
    t = stats.get("batch_done", [])
    if len(t) < 3:
        return float("nan")
    return (len(t) - 1) * batch_size / max(t[-1] - t[0], 1e-9)


@torch.no_grad()
def eval_scenes_rpn(model, cfg, device, source, scene_ids, batch_size=8, output_dir=None, test=False, save_feature=False,
                    stats=None, labels=None, runner=None):
    """--eval_mode rpn over ``scene_ids`` (eval_one_epoch_rpn, eval_rcnn.py:120-260).  Per batch: the RPN stage and proposal layer
    (RpnRunner); unless ``test``, the sources' EVAL-mode gt_boxes3d are packed and the label kernel (csrc/rpn_labels.hip) labels the
    backbone's xyz and counts (correct, fg, pred) per scene; ``stats`` (rpn_eval.RpnStats) takes the counters and the recall of the
    RoIs.  ``output_dir``: the reference's files (detections/data, seg_result, features/ with ``save_feature``), written by writer
    processes.  ``labels``: a list that receives each batch's (ids, cls (B, N) int32 host array).  Returns per scene the host
    (rois, roi_scores_raw) in scene order.  ``runner``: a runner of ``model`` kept by the caller across calls (the checkpoint sweep)."""
    from . import rpn_eval
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    if runner is None:
        runner = make_runner(model, cfg, device)
    thresh = float(cfg.RPN.SCORE_THRESH)
    writers, jobs, out = None, [], []
    if output_dir:
        os.makedirs(os.path.join(output_dir, "detections", "data"), exist_ok=True)
        os.makedirs(os.path.join(output_dir, "seg_result"), exist_ok=True)
        if save_feature:
            os.makedirs(os.path.join(output_dir, "features"), exist_ok=True)
        writers = ProcessPoolExecutor(max_workers=max(1, min(4, host_budget()["writers"])), initializer=_limit_worker_threads,
                                      mp_context=multiprocessing.get_context("forkserver"))

    def finish(det, ids, meta, host_pts, intensity):
        B = len(ids)
        cls = None
        if not test:
            gt_list = [source.gt_boxes3d(i) for i in ids]
            gt, counts, trig = rpn_eval.pack_gt(gt_list)
            counters = torch.zeros((B, 3), dtype=torch.int32, device=device)
            cls, _ = rpn_eval.rpn_labels(det["backbone_xyz"], gt, counts, device=device, want_reg=False, trig=trig,
                                         scores_raw=det["rpn_scores_raw"], thresh=thresh, stats=counters)
            if stats is not None:
                stats.update_seg(counters)
                stats.update_recall(det["rois"], gt_list)
        rois, scores = det["rois"].cpu().numpy(), det["roi_scores_raw"].cpu().numpy()
        out.extend(zip(rois, scores))
        cls_h = cls.cpu().numpy() if cls is not None else None
        if labels is not None and cls_h is not None:
            labels.append((list(ids), cls_h))
        if writers is not None:
            raw = det["rpn_scores_raw"].cpu().numpy()
            pred = rpn_eval.seg_decision(raw, thresh)
            seg, feats = [], [] if save_feature else None
            xyz = det["backbone_xyz"].cpu().numpy()
            fts = det["rpn_features"].cpu().numpy() if save_feature else None
            for k in range(B):
                cols = [host_pts[k][:, :3], pred[k].reshape(-1, 1).astype(np.float32)]
                if cls_h is not None:
                    cols.insert(1, cls_h[k].reshape(-1, 1).astype(np.float32))
                seg.append(np.concatenate(cols, axis=1))
                if save_feature:
                    f = {"": fts[k], "_xyz": xyz[k], "_seg": pred[k].astype(np.float32), "_rawscore": raw[k]}
                    f["_intensity"] = intensity[k]             # pts_features[:, 0] = reflectance - 0.5, (N,) f32
                    feats.append(f)
            jobs.append(writers.submit(_write_rpn_batch, list(ids), [m[0] for m in meta], [m[1] for m in meta], list(rois),
                                       list(scores), seg, feats, output_dir, cfg.CLASSES))

    pending = None
    try:
        for s in range(0, len(scene_ids), batch_size):
            ids = scene_ids[s:s + batch_size]
            if save_feature:
                loaded = [source.load_with_features(i) for i in ids]
                intensity = [l[1] for l in loaded]
                loaded = [(l[0], l[2], l[3]) for l in loaded]
            else:
                loaded, intensity = [source.load(i) for i in ids], None
            host = np.stack([l[0] for l in loaded], 0)
            pts = torch.from_numpy(host).pin_memory().to(device, non_blocking=True)
            det = runner.submit(pts)
            if det is not None:
                finish(det, *pending)
            pending = (ids, [(l[1], l[2]) for l in loaded], host, intensity)
        det = runner.flush()
        if det is not None:
            finish(det, *pending)
        for j in jobs:
            j.result()
    finally:
        if writers is not None:
            writers.shutdown(wait=True, cancel_futures=True)
    return out


class _SceneDataset(torch.utils.data.Dataset):
    """What a loader process produces for scene k: the sampled cloud (host input stage) or the raw cloud (device stage)."""

    def __init__(self, source, scene_ids, raw):
        self.source, self.scene_ids, self.raw = source, list(scene_ids), raw

    def __len__(self):
        return len(self.scene_ids)

    def __getitem__(self, k):
        if self.raw:
            return torch.from_numpy(np.ascontiguousarray(self.source.load_raw(self.scene_ids[k])[0], dtype=np.float32))
        return torch.from_numpy(self.source.load(self.scene_ids[k])[0])


def _identity(items):
    return items


def eval_synthetic(model, cfg, device, scene_ids, batch_size=8, npoints=16384, output_dir=None, raw_points=None):
    """eval_scenes over the synthetic generator (seed = scene id); ``raw_points`` generates denser raw
    clouds that are reduced with the reference's near/far sampler (cross-domain config)."""
    from . import kitti_io
    assert npoints == cfg.RPN.NUM_POINTS, "npoints must equal cfg.RPN.NUM_POINTS"
    src = kitti_io.SyntheticSource(cfg, 0, raw_points=raw_points)
    return eval_scenes(model, cfg, device, src, scene_ids, batch_size, output_dir)


def build_parser():
    ap = argparse.ArgumentParser(description="PointRCNN joint evaluation on synthetic KITTI-shaped scenes (MI355X)")
    ap.add_argument("--cfg_file", type=str, default=None, help="reference-style yaml (tools/cfgs/*.yaml)")
    ap.add_argument("--eval_mode", type=str, default="rcnn")
    ap.add_argument("--ckpt", type=str, default=None, help="reference .pth checkpoint (random init if omitted)")
    ap.add_argument("--rpn_ckpt", type=str, default=None, help="load_part_ckpt after --ckpt: the keys of this file that the model has")
    ap.add_argument("--rcnn_ckpt", type=str, default=None, help="load_part_ckpt after --ckpt and --rpn_ckpt")
    ap.add_argument("--eval_all", action="store_true", help="evaluate every checkpoint of --ckpt_dir that the record file does not list")
    ap.add_argument("--ckpt_dir", type=str, default=None, help="--eval_all: directory of *checkpoint_epoch_*.pth (or a train_rcnn output directory)")
    ap.add_argument("--start_epoch", type=int, default=0, help="--eval_all: skip checkpoints whose epoch id is below this")
    ap.add_argument("--extra_tag", type=str, default="default", help="--eval_all: results go to <output_dir>/eval/eval_all_<extra_tag>")
    ap.add_argument("--wait", type=float, default=None, metavar="SECONDS",
                    help="--eval_all: when no unevaluated checkpoint is left, look again every SECONDS instead of returning")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--scenes", type=int, default=16, help="number of synthetic scenes (ignored with --data_root)")
    ap.add_argument("--raw_points", type=int, default=None,
                    help="synthetic scenes: generate this many raw points per scene (e.g. 180000, the cross-domain "
                         "dense-cloud case) and reduce them with the near/far sampler")
    ap.add_argument("--workers", type=int, default=None, help="host loader processes (default 8)")
    ap.add_argument("--device_input", action="store_true",
                    help="loaders only read raw clouds; rectification, validity filter and the near/far sampler run on the GPU")
    ap.add_argument("--data_root", type=str, default=None, help="directory holding KITTI/object/... and KITTI/ImageSets")
    ap.add_argument("--split", type=str, default=None, help="ImageSets split (default cfg.TEST.SPLIT)")
    ap.add_argument("--output_dir", type=str, default=None)
    ap.add_argument("--eval_ap", action="store_true", help="rank 0: KITTI AP of the gathered detections vs the labels")
    ap.add_argument("--ap_metric", type=str, default="new", choices=["new", "old"],
                    help="--eval_ap difficulty rule: new = distance bands, old = KITTI's bbox-height levels")
    ap.add_argument("--ap_dataset", type=str, default="kitti", choices=["kitti", "argo", "nusc", "lyft", "waymo"],
                    help="--ap_metric old: whose focal length scales the 40 / 25 / 25 px height caps")
    ap.add_argument("--ap_stats_device", type=str, default="cpu", choices=["cpu", "cuda"],
                    help="--eval_ap: flags, matching and PR sums on the host (default) or on the GPU; the same numbers")
    ap.add_argument("--ap_parse_device", type=str, default=None, choices=["cuda", "cpu"],
                    help="--eval_ap: parse the scenes' result texts (and a tree's label files) in one call on the GPU (cuda) or by its "
                         "Python checker (cpu) instead of the host parser (default); the same numbers")
    ap.add_argument("--recall", action="store_true", help="RoI / refined-box recall vs the ground truth (the reference's statistics without --test)")
    ap.add_argument("--save_result", action="store_true", help="--eval_mode rpn: write detections/data and seg_result")
    ap.add_argument("--save_rpn_feature", action="store_true", help="--eval_mode rpn: also write the backbone features (features/)")
    ap.add_argument("--test", action="store_true", help="--eval_mode rpn: no ground truth (no labels, no statistics)")
    ap.add_argument("--set", dest="set_cfgs", default=None, nargs=argparse.REMAINDER)
    return ap


def load_part_ckpts(model, args, log=None):
    """--rpn_ckpt, then --rcnn_ckpt: train_rcnn.load_part_ckpt (the keys of the file that the model has; RuntimeError when none is)"""
    from .train_rcnn import load_part_ckpt
    import logging
    log = log or logging.getLogger("eval_rcnn")
    for name in (args.rpn_ckpt, args.rcnn_ckpt):
        if name:
            load_part_ckpt(model, name, log)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.eval_all and not args.ckpt_dir:
        raise ValueError("eval_rcnn: --eval_all needs --ckpt_dir")
    if args.eval_all and not args.output_dir:
        raise ValueError("eval_rcnn: --eval_all needs --output_dir (the record file and the per-epoch results live under it)")

    cfg = config_mod.make_cfg()
    config_mod.apply_eval_defaults(cfg, args.eval_mode)
    if args.cfg_file:
        config_mod.cfg_from_file(cfg, args.cfg_file)
    if args.set_cfgs:
        config_mod.cfg_from_list(cfg, args.set_cfgs)
    if not torch.cuda.is_available():
        raise RuntimeError("eval_rcnn: no GPU visible; this build has no CPU path")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl")
    model = build_model(cfg, device)
    if args.ckpt:
        load_checkpoint(model, args.ckpt)
    from . import kitti_io
    if args.data_root:
        source = kitti_io.KittiSource(args.data_root, cfg, args.split or cfg.TEST.SPLIT)
    else:
        source = kitti_io.SyntheticSource(cfg, args.scenes, raw_points=args.raw_points)
    my_ids = [source.ids[i] for i in shard_scene_ids(len(source.ids), rank, world)]
    if args.eval_all:
        from . import eval_sweep
        return eval_sweep.sweep(args, model, cfg, device, source, my_ids, rank, world)
    load_part_ckpts(model, args)
    return evaluate_model(args, model, cfg, device, source, my_ids, rank, args.output_dir)


def evaluate_model(args, model, cfg, device, source, my_ids, rank, output_dir, runner=None, labels=None, timings=None,
                   prepared_gt=None):
    """One evaluation of ``model`` as it stands, in the mode of ``args``: what a --ckpt run does behind its checkpoint load, with its
    files under ``output_dir``.  -> the mode's result dictionary (rpn: RpnStats.result(), None with --test; rcnn: scenes, detections,
    the recalls with --recall, the AP dictionary with --eval_ap).  The sweep passes the ``runner`` it keeps, ``labels`` (the source
    behind a label cache, for the AP), ``timings``, a dict that receives the seconds of 'inference' and 'ap', and with
    --ap_stats_device cuda ``prepared_gt``, the labels' table built once (results.prepare_gt)."""
    timings = {} if timings is None else timings
    if args.eval_mode == "rpn":
        t0 = time.perf_counter()
        res = _main_rpn(args, model, cfg, device, source, my_ids, rank, output_dir=output_dir, runner=runner)
        timings["inference"], timings["ap"] = time.perf_counter() - t0, 0.0
        return res
    out = os.path.join(output_dir, "final_result", "data") if output_dir else None
    t0 = time.perf_counter()
    recall = RecallStats(device) if args.recall else None
    stats = {}
    table, counts = eval_scenes(model, cfg, device, source, my_ids, args.batch_size, out, workers=args.workers,
                                device_input=args.device_input, recall=recall, stats=stats, runner=runner)
    elapsed = time.perf_counter() - t0
    res = {}
    if recall is not None:
        res.update(recall.result())
        for k, v in res.items():
            print("rank %d  %s: %s" % (rank, k, v))
    table, counts = all_gather_detections(table, counts, device)
    timings["inference"], timings["ap"] = time.perf_counter() - t0, 0.0
    res.update({"scenes": int(table.shape[0]), "detections": int(counts.sum())})
    if rank == 0:
        print("scenes=%d detections=%d  (%.1f scenes/s on this rank incl. the host input stage%s; steady state %.1f scenes/s, "
              "loader start-up excluded)" %
              (table.shape[0], int(counts.sum()), len(my_ids) / max(elapsed, 1e-9),
               " and the result writer" if out else "", steady_state_rate(stats, args.batch_size)))
        if args.eval_ap:
            t1 = time.perf_counter()
            text, ap = evaluate_detections(table, counts, labels if labels is not None else source, dataset=args.ap_dataset,
                                           device_id=device.index or 0, metric=args.ap_metric,
                                           stats_device=getattr(args, "ap_stats_device", "cpu"), prepared_gt=prepared_gt,
                                           parse_device=getattr(args, "ap_parse_device", None))
            timings["ap"] = time.perf_counter() - t1
            res["ap"] = ap
            print(text)
            if output_dir:
                with open(os.path.join(output_dir, "final_result", "ap.txt"), "w") as f:
                    f.write(text)
    return res


def _main_rpn(args, model, cfg, device, source, my_ids, rank, output_dir=None, runner=None):
    """--eval_mode rpn: eval_scenes_rpn on this rank's scenes and the reference's closing lines.  Returns the statistics dict
    (None with --test).  With more than one rank each rank batches its own shard, so the recall quirk's padding rows (rpn_eval)
    can differ from a single-process run."""
    from . import rpn_eval
    save = args.save_result or args.save_rpn_feature
    result_dir = output_dir or args.output_dir or "."
    stats = None if args.test else rpn_eval.RpnStats(device)
    t0 = time.perf_counter()
    eval_scenes_rpn(model, cfg, device, source, my_ids, args.batch_size, result_dir if save else None, test=args.test,
                    save_feature=args.save_rpn_feature, stats=stats, runner=runner)
    elapsed = time.perf_counter() - t0
    print("rank %d: ---- RPN EVALUATION ---- %d scenes (%.1f scenes/s)" % (rank, len(my_ids), len(my_ids) / max(elapsed, 1e-9)))
    if stats is None:
        return None
    for line in stats.summary_lines(result_dir=result_dir):
        print(line)
    return stats.result()


if __name__ == "__main__":
    main()
