"""The checkpoint sweep of the evaluation driver, ``eval_rcnn --eval_all`` (reference: tools/eval_rcnn.py repeat_eval_ckpt :791-848 and
get_no_evaluated_ckpt :775-788): every checkpoint of --ckpt_dir that the record file does not list yet is evaluated, oldest first.

  python -m 3d_adapt_auto_driving_amd.eval_rcnn --eval_mode rcnn|rpn --eval_all --ckpt_dir D --output_dir O [--start_epoch E]
         [--extra_tag T] [--wait SECONDS] [--rpn_ckpt C] [--rcnn_ckpt C] [--eval_ap] [--recall] [--scenes N | --data_root R] ...

Selection (`unevaluated_ckpts`): the files ``*checkpoint_epoch_*.pth`` of D by modification time; the epoch id is the last match of
``checkpoint_epoch_(.*).pth``, kept as the string it is ("12.5" is legal); a checkpoint is skipped when its id is in the record file
(compared as numbers, as the reference does) or ``int(float(id)) < start_epoch``.  An id that is no number ("best") is skipped: the
reference's float() raises on it.  D may be a train_rcnn output directory: its ``ckpt/`` is taken when D itself holds no checkpoint.

Layout, all under ``O/eval/eval_all_<extra_tag>/`` (the reference's):
  eval_list_<split>.txt       the record: created empty, one id appended per checkpoint AFTER its results are on disk
  log_eval_all_<split>.txt    the log
  epoch_<id>/<split>/         what a single --ckpt run of the mode writes under its --output_dir
  sweep_<split>.jsonl         one line per checkpoint {epoch, ckpt, result, seconds: {load, reload, inference, ap}}, or
                              {epoch, ckpt, skipped: reason}; it stands in for the reference's tensorboard events

ONE difference from the reference: it polls the directory every 30 s for ever.  Here the sweep returns when no unevaluated checkpoint
is left; ``--wait SECONDS`` restores the polling (to follow a training run).

The model, the engine and the runner are built ONCE, from the first checkpoint; every later one is load_state_dict ->
runner.reload_weights() (net/fast_infer.py: the folded weights are rewritten through the tensors the engine owns, no graph is
captured again).  --rpn_ckpt / --rcnn_ckpt are applied on top of every checkpoint, in that order.  A checkpoint that cannot be read or
whose tensors do not have the model's shapes is logged, written to the jsonl as skipped and NOT recorded: nothing of the model is
touched by it, and a later run tries it again.  The scene source is opened once; the label lines the AP reads are kept."""
import glob
import json
import logging
import os
import re
import time


def unevaluated_ckpts(ckpt_dir, record_file, start_epoch=0):
    """-> [(epoch id, path)] of the checkpoints still to evaluate, in the order get_no_evaluated_ckpt would hand them out one by one"""
    files = glob.glob(os.path.join(ckpt_dir, "*checkpoint_epoch_*.pth"))
    files.sort(key=os.path.getmtime)
    done = set()
    if os.path.isfile(record_file):
        with open(record_file) as f:
            for line in f:
                if line.strip():
                    done.add(float(line.strip()))
    out = []
    for path in files:
        ids = re.findall("checkpoint_epoch_(.*).pth", path)
        if not ids:
            continue
        try:
            number = float(ids[-1])
        except ValueError:
            continue
        if number in done or int(number) < start_epoch:
            continue
        out.append((ids[-1], path))
    return out


def get_no_evaluated_ckpt(ckpt_dir, record_file, start_epoch=0):
    """the reference's call: -> (epoch id, path) of the oldest unevaluated checkpoint, or (-1, None)"""
    todo = unevaluated_ckpts(ckpt_dir, record_file, start_epoch)
    return todo[0] if todo else (-1, None)


def resolve_ckpt_dir(d):
    """--ckpt_dir may name a train_rcnn output directory: its ckpt/ holds the checkpoints"""
    sub = os.path.join(d, "ckpt")
    if os.path.isdir(sub) and not glob.glob(os.path.join(d, "*checkpoint_epoch_*.pth")):
        return sub
    return d


def misfit(model, state):
    """-> a message naming the first key of ``state`` that a strict load_state_dict into ``model`` would refuse, or None.  Checked
    BEFORE the load: load_state_dict copies tensor by tensor and would leave the model half loaded."""
    own = model.state_dict()
    missing = [k for k in own if k not in state]
    extra = [k for k in state if k not in own]
    if missing or extra:
        return "missing keys %s, unexpected keys %s" % (missing[:3], extra[:3])
    for k, v in own.items():
        if tuple(state[k].shape) != tuple(v.shape):
            return "%s has shape %s, the model's is %s" % (k, tuple(state[k].shape), tuple(v.shape))
    return None


class _LabelCache:
    """the scene source with its label lines kept: the AP of every checkpoint reads the same label files"""

    def __init__(self, source):
        self._source, self._lines = source, {}

    def label_lines(self, i):
        if i not in self._lines:
            self._lines[i] = self._source.label_lines(i)
        return self._lines[i]

    def __getattr__(self, name):
        if name.startswith("__") or name in ("_source", "_lines"):
            raise AttributeError(name)
        return getattr(self._source, name)


def _jsonable(v):
    import numpy as np
    if isinstance(v, dict):
        return {str(k): _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if hasattr(v, "tolist") and hasattr(v, "dtype"):            # a tensor
        return v.tolist()
    return v


def sweep(args, model, cfg, device, source, my_ids, rank=0, world=1):
    """eval_rcnn.main's --eval_all branch.  -> the list of jsonl entries this call wrote (every rank returns them)"""
    import torch
    from . import eval_rcnn as E
    split = args.split or cfg.TEST.SPLIT
    root = os.path.join(args.output_dir, "eval", "eval_all_" + args.extra_tag)
    os.makedirs(root, exist_ok=True)
    ckpt_dir = resolve_ckpt_dir(args.ckpt_dir)
    if not os.path.isdir(ckpt_dir):
        raise FileNotFoundError(ckpt_dir)
    record = os.path.join(root, "eval_list_%s.txt" % split)
    jsonl = os.path.join(root, "sweep_%s.jsonl" % split)
    if rank == 0:
        with open(record, "a"):
            pass
    if world > 1:
        torch.distributed.barrier()
    log = logging.getLogger("eval_rcnn.sweep.%s" % os.path.abspath(root))
    log.setLevel(logging.INFO)
    log.propagate = False
    handlers = [logging.StreamHandler()] + ([logging.FileHandler(os.path.join(root, "log_eval_all_%s.txt" % split))] if rank == 0 else [])
    for h in handlers:
        h.setFormatter(logging.Formatter("%(asctime)s  %(levelname)5s  %(message)s"))
        log.addHandler(h)
    entries = []

    def write(entry):
        entries.append(entry)
        if rank == 0:
            with open(jsonl, "a") as f:
                f.write(json.dumps(_jsonable(entry)) + "\n")

    try:
        log.info("**********************Start logging**********************")
        for key, val in sorted(vars(args).items()):
            log.info("%-16s %s", key, val)
        labels = _LabelCache(source)
        prepared_gt = None             # the device AP path: the labels' half of the split table, built once for every checkpoint
        if rank == 0 and args.eval_ap and args.eval_mode != "rpn" and getattr(args, "ap_stats_device", "cpu") == "cuda":
            prepared_gt = E.prepare_gt(labels, sorted(source.ids), parse_device=getattr(args, "ap_parse_device", None),
                                       device_id=device.index or 0)
        runner = None
        failed = {}                    # path -> modification time at the failed attempt: tried again only once the file has changed
        clock = time.perf_counter
        while True:
            todo = [(e, p) for e, p in unevaluated_ckpts(ckpt_dir, record, args.start_epoch) if failed.get(p) != os.path.getmtime(p)]
            if not todo:
                if args.wait is None:
                    break
                log.info("Wait %s second for next check: %s", args.wait, ckpt_dir)
                time.sleep(args.wait)
                continue
            epoch, path = todo[0]
            t0 = clock()
            try:
                ckpt = torch.load(path, map_location="cpu", weights_only=False)
                state = ckpt["model_state"] if isinstance(ckpt, dict) and "model_state" in ckpt else ckpt
                if not isinstance(state, dict):
                    raise TypeError("no state dictionary in the file")
                bad = misfit(model, state)
            except Exception as e:                                  # noqa: BLE001 -- a truncated or foreign file must not stop the sweep
                bad = "cannot be read (%s: %s)" % (type(e).__name__, e)
            if bad:
                log.warning("Epoch %s (%s) skipped: %s", epoch, path, bad)
                failed[path] = os.path.getmtime(path)
                write({"epoch": epoch, "ckpt": path, "skipped": bad})
                continue
            t1 = clock()
            if runner is not None:
                while runner.flush() is not None:                   # (an evaluation that raised may have left batches behind)
                    pass
            model.load_state_dict(state)
            E.load_part_ckpts(model, args, log)
            if runner is None:
                runner = E.make_runner(model, cfg, device)           # the engine folds here; graphs are captured with the first batch
            else:
                runner.reload_weights()
            torch.cuda.synchronize(device)
            t2 = clock()
            out_dir = os.path.join(root, "epoch_%s" % epoch, split)
            os.makedirs(out_dir, exist_ok=True)
            timings = {}
            result = E.evaluate_model(args, model, cfg, device, source, my_ids, rank, out_dir, runner=runner, labels=labels,
                                      timings=timings, prepared_gt=prepared_gt)
            seconds = {"load": t1 - t0, "reload": t2 - t1, "inference": timings.get("inference", 0.0), "ap": timings.get("ap", 0.0)}
            write({"epoch": epoch, "ckpt": path, "result": result, "seconds": {k: round(v, 4) for k, v in seconds.items()}})
            if rank == 0:
                with open(record, "a") as f:                         # only now: the results are on disk
                    f.write("%s\n" % epoch)
            if world > 1:
                torch.distributed.barrier()                          # every rank reads the record for its next choice
            log.info("Epoch %s has been evaluated (load %.3f s, reload %.3f s, inference %.3f s, ap %.3f s)", epoch,
                     seconds["load"], seconds["reload"], seconds["inference"], seconds["ap"])
    finally:
        for h in handlers:
            log.removeHandler(h)
            h.close()
    return entries
