"""The train loop (reference: tools/train_rcnn.py with TRAIN.OPTIMIZER 'adam_onecycle' and tools/train_utils/train_utils.py
Trainer.train / checkpoint_state / load_checkpoint / load_part_ckpt): a KITTI-format tree and a GT database -> checkpoints.

  python -m 3d_adapt_auto_driving_amd.train_rcnn --train_mode rpn|rcnn --root R [--gt_database DB.pkl] [--cfg_file Y] [--batch_size 16]
         [--epochs 200] [--ckpt_save_interval 5] [--ckpt C] [--rpn_ckpt C] [--npoints_faraway 4000] [--output_dir D] [--seed S]
         [--device cuda|cpu] [--ordered_backward] [--fused_layers] [--engine_rpn] [--subsample N] [--shuffle_subsample S]
         [--with_replace] [--rcnn_ckpt C] [--set K V ...]

``rpn`` trains the first stage alone (RPN.ENABLED, RCNN off); ``rcnn`` trains the second stage on a fixed first one (RCNN.ENABLED,
RPN.ENABLED = RPN.FIXED = True; the RPN's parameters are frozen AFTER the optimizer is built, so they keep their places in its groups).
total_steps = len(loader) x epochs, with len(loader) = len(split) // batch_size (the last short batch is dropped).

Per epoch: the BatchNorm momentum from the GLOBAL iteration (as bnm_scheduler.step(it)), then a seeded permutation of the split.
Per iteration: schedule(it), zero_grad, RpnTrainInput.batch -> losses.model_fn -> backward -> OneCycleAdam.step().
Outputs under --output_dir: ckpt/checkpoint_epoch_N.pth = {'epoch', 'it', 'model_state', 'optimizer_state'} every --ckpt_save_interval
epochs (the reference's layout: either side resumes the other's file), log_train.txt, and train_log.jsonl with one line per iteration
{it, epoch, lr, loss, grad_norm, the tb_dict entries}: it stands in for the reference's tensorboard events ('it' counts finished
iterations, as the reference's event step does; 'lr' is the rate that iteration ran with).
--ckpt resumes the model, the optimizer, 'it' and 'epoch'; --rpn_ckpt is load_part_ckpt (the keys the model has).
--device cpu selects the checker paths of the input stage, the losses and the optimizer; the model's operators exist for CUDA tensors
only, so a cpu run needs the test suite's stand-ins for them and is of use to tests alone.  --set K V ... (last on the line) overrides
configuration keys, as in eval_rcnn.  --ordered_backward runs every backward of the grouping, gather and interpolation operators through
the order-fixed sums (pointnet2_utils.ORDERED_BACKWARD, csrc/scatter_plan.hip) and says so in one line of log_train.txt; without it no
file differs from what the loop wrote before the flag existed.  The claim is about THIS project's operators: torch's own convolution and
batch-norm backward are not covered by it.  --fused_layers runs every covered conv + BatchNorm + ReLU block of the model in training mode
(pointnet2/train_layer.py covers()) forward and backward on the project's own order-fixed kernels (pytorch_utils.FUSED_TRAIN_LAYERS,
csrc/train_layer.hip) instead of torch's modules, and says so in one line of log_train.txt; without it no file differs either.  Blocks in
eval mode (the fixed RPN of --train_mode rcnn) run torch's modules as before.  --engine_rpn (--train_mode rcnn only; with rpn it raises
ValueError before anything is written) runs that fixed first stage on the inference engine instead of the module graph
(net/frozen_rpn.py FrozenFirstStage: backbone, heads, proposal layer at the TRAIN quotas as HIP kernels over weights folded once, after
--ckpt / --rpn_ckpt are loaded) and says so in one line of log_train.txt; a configuration the engine does not cover raises by name, there
is no fall-back.  Checkpoints keep their layout: model.state_dict() still holds the RPN's own tensors, untouched.  Without it no file differs.

Data-parallel (dist_train.py): started under a launcher that sets RANK, WORLD_SIZE and LOCAL_RANK, e.g.
  torchrun --nproc_per_node 8 -m 3d_adapt_auto_driving_amd.train_rcnn --train_mode rpn ... [--dist_backend nccl|gloo]
the loop is one rank per GPU with nn.DataParallel's semantics: --batch_size is the GLOBAL batch (B % W != 0 raises ValueError before
anything is written), every rank draws the same epoch permutation and takes its contiguous B / W rows of each batch, the loss is the whole
batch's (the rows it reads are gathered over the ranks), parameter gradients are summed in one packed exchange and every rank applies
the same step.  Only rank 0 writes ckpt/, log_train.txt and train_log.jsonl (one more line in the Start logging block names the world
size and the backend); rank 0's BatchNorm buffers are the checkpoint's; the replicas' parameter digests are compared before every
checkpoint and at the end, and a difference raises instead of saving.  torch.manual_seed(seed) is the same on every rank and rank 0's
tensors are broadcast once after --ckpt / --rpn_ckpt are loaded; the per-rank random streams (augmentation, RoI sampling) are seeded
seed + rank, so a W-rank run is NOT the sample stream of a 1-rank run.  Without the launcher's variables, or with WORLD_SIZE=1, there is
no process group and no file differs from what the loop wrote before.

Few-shot fine-tuning (the reference's tools/train_rcnn.py:50-54; README "Few-shot fine-tuning" has the whole chain): --subsample N trains
on the first N ids of KITTI/ImageSets/train_car1.txt (car_split.py writes it), or of train_car1_<S>.txt with --shuffle_subsample S, which
scene_batch.sample_id_list writes from an UNSEEDED shuffle when it is missing; the object filter of the input stage follows, as on any
list.  It needs TRAIN.SPLIT train: with another split the reference ignores the flag and trains on the full split, here that is a
ValueError before anything is written.  Under a process group rank 0 alone resolves (and, if need be, writes) the list and every rank is
handed rank 0's (resolve_sample_ids), so the replicas cannot train on different lists.  One more line in the Start logging block names
the list file, the count after the cut, the count after the object filter and the ids.  Fewer samples than one batch is the error it
always was (--subsample 10 --batch_size 16).  --with_replace is the near-point sampler's ``replace`` (RpnTrainInput with_replace).
--rcnn_ckpt is load_part_ckpt, applied after --rpn_ckpt and before the broadcast and the engine fold: the keys the file shares with the
model are taken from it, so a whole pretrained PointRCNN goes in through either flag.  (The reference's trainer names a
load_rcnn_part_ckpt that does not exist, so the flag raises there as shipped; this is the meaning eval_rcnn gives it.)  The four flags
are absent from the namespace unless given: a run without them writes the log_train.txt it always wrote.

Random object scaling (README "Random object scaling"; object_scale.py): --obj_scale LO HI [--obj_scale_prob P] hands both values to
RpnTrainInput in either train mode: every iteration each labelled object's points and box are rescaled by a factor of its own, drawn from
a random stream of its own.  One line of log_train.txt names range and probability, and every line of train_log.jsonl gains
``objects_scaled`` (final gt boxes of the writer's rows whose factor is not 1) and ``objects_without_points`` (those that own no point).
Both flags are absent from the namespace unless given, and no config key exists for them: a run without them writes what it always wrote.

Out of scope, each raising NotImplementedError with its own name before anything is written: --mgpus (DataParallel inside one process;
the launcher form above is its counterpart), --train_with_eval,
--train_mode rcnn_offline, TRAIN.OPTIMIZER 'adam' and 'sgd' (with their LambdaLR and warm-up schedulers).
"""
import argparse
import json
import logging
import os

import numpy as np


def load_part_ckpt(model, filename, log):
    import torch
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    state = torch.load(filename, map_location="cpu", weights_only=False)["model_state"]
    own = model.state_dict()
    update = {k: v for k, v in state.items() if k in own}
    if not update:
        raise RuntimeError("train_rcnn: %s holds no key of this model" % filename)
    own.update(update)
    model.load_state_dict(own)
    log.info("==> Done (loaded %d/%d)" % (len(update), len(own)))


def load_part_ckpts(model, a, log):
    """--rpn_ckpt, then --rcnn_ckpt: a key both files hold ends with the second file's value"""
    for flag in ("rpn_ckpt", "rcnn_ckpt"):
        if getattr(a, flag, None) is not None:
            load_part_ckpt(model, getattr(a, flag), log)


def load_checkpoint(model, optimizer, filename, log):
    """-> (it, epoch)"""
    import torch
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    log.info("==> Loading from checkpoint '%s'" % filename)
    ckpt = torch.load(filename, map_location="cpu", weights_only=False)
    if ckpt.get("model_state") is not None:
        model.load_state_dict(ckpt["model_state"])
    if ckpt.get("optimizer_state") is not None:
        optimizer.load_state_dict(ckpt["optimizer_state"])
    return int(ckpt.get("it", 0)), int(ckpt.get("epoch", -1))


def save_checkpoint(model, optimizer, epoch, it, filename):
    import torch
    torch.save({"epoch": epoch, "it": it, "model_state": model.state_dict(), "optimizer_state": optimizer.state_dict()}, filename)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.train_rcnn", description=__doc__.split("\n")[0])
    ap.add_argument("--train_mode", type=str, required=True)
    ap.add_argument("--root", type=str, required=True)
    ap.add_argument("--gt_database", type=str, default=None)
    ap.add_argument("--cfg_file", type=str, default=None)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--ckpt_save_interval", type=int, default=5)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--rpn_ckpt", type=str, default=None)
    ap.add_argument("--npoints_faraway", type=int, default=4000)
    ap.add_argument("--output_dir", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--mgpus", action="store_true")
    ap.add_argument("--train_with_eval", action="store_true")
    ap.add_argument("--ordered_backward", action="store_true")
    ap.add_argument("--fused_layers", action="store_true")
    ap.add_argument("--engine_rpn", action="store_true")
    # (absent from the namespace unless given: a run without it logs the arguments it always logged)
    ap.add_argument("--dist_backend", type=str, default=argparse.SUPPRESS, choices=("nccl", "gloo"))
    ap.add_argument("--subsample", type=int, default=argparse.SUPPRESS)
    ap.add_argument("--shuffle_subsample", type=str, default=argparse.SUPPRESS)
    ap.add_argument("--with_replace", action="store_true", default=argparse.SUPPRESS)
    ap.add_argument("--rcnn_ckpt", type=str, default=argparse.SUPPRESS)
    ap.add_argument("--obj_scale", type=float, nargs=2, metavar=("LO", "HI"), default=argparse.SUPPRESS)
    ap.add_argument("--obj_scale_prob", type=float, default=argparse.SUPPRESS)
    ap.add_argument("--set", dest="set_cfgs", default=None, nargs=argparse.REMAINDER)
    return ap


def make_cfg(a):
    """The configuration of a run; raises for what is out of scope"""
    from . import config
    if a.mgpus:
        raise NotImplementedError("train_rcnn: --mgpus (nn.DataParallel inside one process) is out of scope; start one process per GPU under a "
                                  "launcher instead (torchrun --nproc_per_node N -m 3d_adapt_auto_driving_amd.train_rcnn ...)")
    if a.train_with_eval:
        raise NotImplementedError("train_rcnn: --train_with_eval is out of scope")
    if a.train_mode == "rcnn_offline":
        raise NotImplementedError("train_rcnn: --train_mode rcnn_offline is out of scope")
    if a.train_mode not in ("rpn", "rcnn"):
        raise NotImplementedError("train_rcnn: --train_mode %r" % (a.train_mode,))
    if getattr(a, "engine_rpn", False) and a.train_mode != "rcnn":
        raise ValueError("train_rcnn: --engine_rpn runs the FIXED first stage of --train_mode rcnn on the inference engine; "
                         "--train_mode %s trains the RPN" % a.train_mode)
    cfg = config.make_cfg()
    config.apply_train_defaults(cfg, a.train_mode)
    if a.gt_database:
        cfg["GT_AUG_ENABLED"], cfg["GT_AUG_RAND_NUM"], cfg["GT_AUG_APPLY_PROB"] = True, True, 1.0      # what the shipped yamls set
    if a.cfg_file:
        config.cfg_from_file(cfg, a.cfg_file)
        cfg.TAG = os.path.splitext(os.path.basename(a.cfg_file))[0]
    if a.set_cfgs:
        config.cfg_from_list(cfg, a.set_cfgs)
    if a.train_mode == "rpn":                                 # the mode wins over the file, as in the reference
        cfg.RPN.ENABLED, cfg.RCNN.ENABLED = True, False
    else:
        cfg.RCNN.ENABLED = True
        cfg.RPN.ENABLED = cfg.RPN.FIXED = True
    if cfg.TRAIN.OPTIMIZER != "adam_onecycle":
        raise NotImplementedError("train_rcnn: TRAIN.OPTIMIZER %r is out of scope (adam_onecycle is what this loop runs)" % (cfg.TRAIN.OPTIMIZER,))
    if getattr(a, "subsample", -1) > 0 and cfg.TRAIN.SPLIT != "train":
        raise ValueError("train_rcnn: --subsample %d cuts train_car1.txt, the few-shot list of the 'train' split, but TRAIN.SPLIT is %r "
                         "(the reference would silently train on the full split)" % (a.subsample, cfg.TRAIN.SPLIT))
    if getattr(a, "engine_rpn", False):                       # what the configuration alone decides, before anything is written
        from .net import frozen_rpn
        frozen_rpn.check_cfg(cfg, "TRAIN")
    return cfg


def logged_args(a):
    """The (key, value) lines of the Start logging block.  The switches named here are logged by lines of their own, and only when set;
    the few-shot flags are absent from the namespace unless given: a run without any of them writes what it always wrote."""
    return [(k, v) for k, v in vars(a).items() if k not in ("ordered_backward", "fused_layers", "engine_rpn", "dist_backend", "obj_scale", "obj_scale_prob")]


def resolve_sample_ids(a, cfg, group=None):
    """-> (the sample list of a --subsample run as RpnTrainInput's ``sample_ids``, the file it came from), or (None, None) without
    --subsample.  Under an active process group rank 0 alone calls scene_batch.sample_id_list -- which WRITES a missing
    train_car1_<S>.txt from an unseeded shuffle -- and every rank returns rank 0's list; a failure there raises on every rank."""
    from .scene_batch import sample_id_list, sample_list_file
    subsample, shuffle = getattr(a, "subsample", -1), getattr(a, "shuffle_subsample", None)
    if subsample <= 0:
        return None, None
    path = sample_list_file(a.root, cfg.TRAIN.SPLIT, subsample, shuffle)
    ids = error = None
    if group is None or not group.active or group.rank == 0:
        try:
            ids = sample_id_list(a.root, cfg.TRAIN.SPLIT, subsample, shuffle)
        except OSError as e:
            if group is None or not group.active:
                raise
            error = "%s: %s" % (type(e).__name__, e)
    if group is not None and group.active:
        ids, error = group.broadcast_object((ids, error))
        if error is not None:
            raise RuntimeError("train_rcnn: rank 0 could not read the --subsample list %s (%s)" % (path, error))
    return ids, path


def main(argv=None):
    a = build_parser().parse_args(argv)
    cfg = make_cfg(a)
    import contextlib
    import torch
    from . import dist_train, losses, optim
    rank, world, _local = dist_train.world_from_env()
    if a.batch_size % world:                                  # before anything is written
        raise ValueError("train_rcnn: --batch_size %d is the GLOBAL batch and does not divide over WORLD_SIZE=%d" % (a.batch_size, world))
    from .pointnet2 import pointnet2_utils, pytorch_utils
    from .net.point_rcnn import PointRCNN
    from .train_input import RpnTrainInput, check_obj_scale, obj_scale_args
    ros = obj_scale_args(a)                                   # before anything is written
    check_obj_scale(ros.get("obj_scale"), ros.get("obj_scale_prob", 1.0))

    out_dir = a.output_dir or os.path.join("output", a.train_mode, cfg.TAG)
    ckpt_dir = os.path.join(out_dir, "ckpt")
    writer = rank == 0                                        # only rank 0 writes ckpt/, log_train.txt and train_log.jsonl
    if writer:
        os.makedirs(ckpt_dir, exist_ok=True)
    log = logging.getLogger("train_rcnn.%s%s" % (os.path.abspath(out_dir), "" if writer else ".rank%d" % rank))
    log.setLevel(logging.INFO)
    log.propagate = False
    handlers = [logging.FileHandler(os.path.join(out_dir, "log_train.txt")), logging.StreamHandler()] if writer else [logging.NullHandler()]
    group = None
    for h in handlers:
        h.setFormatter(logging.Formatter("%(asctime)s  %(levelname)5s  %(message)s"))
        log.addHandler(h)
    try:
        log.info("**********************Start logging**********************")
        for key, val in logged_args(a):
            log.info("{:16} {}".format(key, val))
        if a.ordered_backward:
            log.info("ordered_backward True: grouping / gather / interpolate gradients are summed in a fixed order (no float atomics)")
        if a.fused_layers:
            log.info("fused_layers True: conv + BatchNorm + ReLU blocks in training mode run the order-fixed training layer (forward and backward)")
        group = dist_train.ReplicaGroup.from_env(a.device, getattr(a, "dist_backend", None))
        if group.active:
            log.info("world_size %d backend %s: data-parallel, one rank per GPU; --batch_size %d is the global batch, %d rows per rank; "
                     "gradients are summed in one packed exchange" % (world, group.backend, a.batch_size, a.batch_size // world))
        sample_ids, list_file = resolve_sample_ids(a, cfg, group)
        src = RpnTrainInput(a.root, cfg, a.gt_database, split=cfg.TRAIN.SPLIT, classes=cfg.CLASSES, npoints=cfg.RPN.NUM_POINTS,
                            npoints_faraway=a.npoints_faraway, with_replace=getattr(a, "with_replace", False),
                            seed=a.seed + rank if group.active else a.seed, device=a.device, sample_ids=sample_ids, **ros)
        if ros:
            log.info("obj_scale %g %g prob %g: every labelled object's points and box are rescaled by a factor of its own per iteration" %
                     (src.obj_scale + (src.obj_scale_prob,)))
        if sample_ids is not None:
            log.info("subsample %d: %s -> %d ids, %d after the object filter: %s" %
                     (a.subsample, list_file, len(sample_ids), len(src), " ".join("%06d" % i for i in src.sample_id_list)))
        per_epoch = len(src) // a.batch_size
        if per_epoch < 1:
            raise ValueError("train_rcnn: the split holds %d samples, fewer than one batch of %d" % (len(src), a.batch_size))
        torch.manual_seed(a.seed)
        model = PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN").to(a.device)
        T = cfg.TRAIN
        opt = optim.OneCycleAdam(model, per_epoch * a.epochs, T.LR, list(T.MOMS), T.DIV_FACTOR, T.PCT_START, T.WEIGHT_DECAY, T.GRAD_NORM_CLIP,
                                 group=group)
        if cfg.RPN.ENABLED and cfg.RPN.FIXED:                 # after the optimizer is built: the groups keep the RPN's parameters
            for p in model.rpn.parameters():
                p.requires_grad = False
        it = start_epoch = 0
        if a.ckpt is not None:
            it, start_epoch = load_checkpoint(model, opt, a.ckpt, log)
            log.info("==> resumed at epoch %d, it %d" % (start_epoch, it))
        load_part_ckpts(model, a, log)
        if group.active:                                      # after the loads: every replica starts from rank 0's tensors
            group.broadcast_model(model)
            if cfg.RCNN.ENABLED:
                model.rcnn_net.target_seed = a.seed + rank
        if a.engine_rpn:                                      # after the loads: it folds the weights that will be used
            from .net.frozen_rpn import FrozenFirstStage
            model.use_engine_first_stage(FrozenFirstStage(model, cfg))
            log.info("engine_rpn True: the fixed first stage runs on the inference engine (weights folded once, proposal layer at the TRAIN quotas)")
        order = np.random.RandomState(a.seed)
        for _ in range(start_epoch):                          # the permutations of the epochs already trained
            order.permutation(len(src))
        log.info("**********************Start training**********************")
        model.train()
        ordered = pointnet2_utils.ordered_backward(True) if a.ordered_backward else contextlib.nullcontext()
        fused = pytorch_utils.fused_train_layers(True) if a.fused_layers else contextlib.nullcontext()
        sink = open(os.path.join(out_dir, "train_log.jsonl"), "a") if writer else contextlib.nullcontext()
        with ordered, fused, sink as events:
            for epoch in range(start_epoch, a.epochs):
                optim.set_bn_momentum(model, optim.bn_momentum(cfg, it))
                perm = order.permutation(len(src))
                for k in range(per_epoch):
                    opt.schedule(it)
                    lr = opt.lr
                    opt.zero_grad()
                    batch = src.batch(group.shard(perm[k * a.batch_size:(k + 1) * a.batch_size]))
                    if group.active:
                        loss, tb_dict, disp_dict = dist_train.model_fn_replicas(cfg, model, batch, group)
                    else:
                        loss, tb_dict, disp_dict = losses.model_fn(cfg, model, batch)
                    loss.backward()
                    opt.step()
                    it += 1
                    line = dict(it=it, epoch=epoch, lr=lr, loss=float(loss.detach()), grad_norm=float(opt.total_norm), **tb_dict)
                    if ros:
                        line["objects_scaled"] = sum(1 for rec in src.last_scaled if rec[2] != 1.0)
                        line["objects_without_points"] = sum(1 for rec in src.last_scaled if rec[3] == 0)
                    if writer:
                        events.write(json.dumps(line) + "\n")
                        events.flush()
                    log.info("epoch %d it %d lr %.6e %s" % (epoch, it, lr, " ".join("%s %.4f" % kv for kv in sorted(disp_dict.items()))))
                trained = epoch + 1
                if trained % a.ckpt_save_interval == 0:
                    if group.active:                          # replicas that drifted raise here, on every rank, instead of saving
                        group.digest_check(model.parameters())
                    if writer:
                        save_checkpoint(model, opt, trained, it, os.path.join(ckpt_dir, "checkpoint_epoch_%d.pth" % trained))
            if group.active:
                group.digest_check(model.parameters())
        log.info("**********************End training**********************")
    finally:
        if group is not None:
            group.close()
        for h in handlers:
            log.removeHandler(h)
            h.close()
    return it


if __name__ == "__main__":
    main()
