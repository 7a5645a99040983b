"""The weight step of training (reference: tools/train_utils/train_utils.py Trainer._train_it, tools/train_utils/fastai_optim.py
OptimWrapper, tools/train_utils/learning_schedules_fastai.py OneCycle, tools/train_rcnn.py create_optimizer / create_scheduler with
TRAIN.OPTIMIZER 'adam_onecycle'): gradient-norm clip, decoupled weight decay, Adam, the one-cycle schedule of lr and beta1, and the
BatchNorm momentum schedule.

  opt = OneCycleAdam(model, total_steps, lr_max, moms, div_factor, pct_start, wd, grad_norm_clip)
  for it in range(total_steps):
      opt.schedule(it);  opt.zero_grad();  loss.backward();  opt.step()
  opt.lr, opt.mom, opt.total_norm, opt.steps_done;  opt.state_dict() / opt.load_state_dict(sd)

What one step() computes, in this order:
  total_norm = sqrt(sum of squares over every parameter of the model that has a grad);  coef = min(1, clip / (total_norm + 1e-6))
  every parameter of the two groups with requires_grad (its grad may be None):  p *= 1 - wd lr
  every such parameter whose grad is not None (state is created on its first such step):  g = grad coef,  step += 1,
      m += (g - m)(1 - beta1),  v = beta2 v + (1 - beta2) g g,  p -= lr / (1 - beta1^step) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
  with beta1 the scheduled ``mom`` of this iteration and ``step`` the parameter's own count: what the installed torch.optim.Adam computes
  when the reference's wrapper drives it.  A parameter frozen after construction (RPN.FIXED) keeps its place in its group, is never
  touched and gets no state (zero_grad() leaves it without a grad).

CUDA parameters run csrc/optim.hip: three launches for the whole model whatever its number of tensors, f64 arithmetic on the f32 state
with one rounding per stored value, sums of a fixed shape (the same input gives the same bits), nothing read back; ``total_norm`` is a
0-dim f64 view of the device workspace, valid after step().  The tensors are described to the kernels by a table of device arrays that
is rebuilt and uploaded only when its host-side signature changes (the parameter and grad addresses, requires_grad, grad is None);
otherwise a step uploads nothing.  THE ONE VISIBLE DIFFERENCE from clip_grad_norm_: grads are read and never written, ``p.grad`` after
step() is the unclipped grad.
CPU parameters run the checker, which is literally torch.nn.utils.clip_grad_norm_, the wrapper's decay loop and
torch.optim.Adam(foreach=False) driven as OptimWrapper drives them; it is not a second product path and neither path falls back to the
other.  The checker also accepts f64 parameters (the tests take the rounding scale of an output from an f32 and an f64 run of it).

OneCycleAdam(..., group=dist_train.ReplicaGroup) is the data-parallel step: the grads are SUMMED over the group's ranks before the step
above, and the clip norm is the sum's.  CUDA: the table gains the columns ``src`` (the tensors' own grads) and ``slot_start``, its grad
column points into one flat f32 bucket, and step() is prcnn_grad_pack (csrc/grad_bucket.hip, one launch) -> ONE all-reduce of the bucket
-> the same three launches reading the reduced grads from the bucket; ``p.grad`` stays the rank's own, and the bucket and table are
rebuilt only with the signature.  CPU: every ``p.grad`` is all-reduced in place before the checker's step.  A group that is not active
(a world of 1) changes nothing.

state_dict() has the layout torch.optim.Adam gives under the reference's wrapper -- two param_groups (non-BatchNorm, BatchNorm) with the
installed Adam's keys, lr, betas = (mom, betas2), weight_decay = 0; state[i] = {step, exp_avg, exp_avg_sq} keyed by the parameter's
index over both groups -- so a checkpoint written here resumes under the reference's load_checkpoint and the other way round.
"""
import ctypes as C

import numpy as np

from . import _lib

CHUNK = _lib.PRCNN_OPTIM_CHUNK          # elements of one tensor per workgroup (csrc/optim.hip)
FLAG_DECAY, FLAG_ADAM = 1, 2


# ------------------------------------------------------------------------------------------------------------------------ schedules
def one_cycle(step, total_steps, lr_max, moms, div_factor, pct_start):
    """OneCycle.step(step) -> (lr, mom), in f64.  Two cosine phases over [0, a) and [a, total_steps) with a = int(pct_start total_steps):
    lr lr_max / div_factor -> lr_max -> lr_max / div_factor / 1e4, mom moms[0] -> moms[1] -> moms[0]; a later phase overrides from its
    start on.  Like the reference it raises ZeroDivisionError where a phase that has begun is empty (a = 0)."""
    low = lr_max / div_factor
    a = int(pct_start * total_steps)
    lr, mom = low, moms[0]                                    # what OneCycle.__init__ sets
    cos = lambda start, end, pct: float(end + (start - end) / 2 * (np.cos(np.pi * pct) + 1))
    for (first, last), (lr0, lr1), (m0, m1) in (((0, a), (low, lr_max), (moms[0], moms[1])),
                                                ((a, total_steps), (lr_max, low / 1e4), (moms[1], moms[0]))):
        if step >= first:
            pct = (step - first) / (last - first)
            lr, mom = cos(lr0, lr1, pct), cos(m0, m1, pct)
    return lr, mom


def bn_momentum(cfg, epoch):
    """create_scheduler's bnm_lmbd (the reference steps it with the global iteration: Trainer.train bnm_scheduler.step(it))"""
    T = cfg.TRAIN
    decay = 1
    for decay_step in T.BN_DECAY_STEP_LIST:
        if epoch >= decay_step:
            decay = decay * T.BN_DECAY
    return max(T.BN_MOMENTUM * decay, T.BNM_CLIP)


def _bn_types():
    import torch.nn as nn
    return (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)


def set_bn_momentum(model, momentum):
    for m in model.modules():
        if isinstance(m, _bn_types()):
            m.momentum = momentum


# --------------------------------------------------------------------------------------------------------------------------- groups
def _leaves(m):
    kids = list(m.children())
    order = getattr(m, "REFERENCE_CHILD_ORDER", None)         # a module whose children the reference registers in another order
    if order:
        named = dict(m.named_children())
        kids = [named[k] for k in order if k in named] + [c for k, c in named.items() if k not in order]
    return sum((_leaves(k) for k in kids), []) if kids else [m]


def layer_groups(model):
    """split_bn_bias([nn.Sequential(*flatten_model(model))]) as two parameter lists: [parameters of the non-BatchNorm leaf modules in
    module order, parameters of the BatchNorm leaf modules]; a parameter met twice is listed once, as Module.parameters() lists it.
    Module order is the REFERENCE's registration order (RCNNNet.REFERENCE_CHILD_ORDER): state_dict() keys the state by index."""
    groups, seen = ([], []), set()
    for leaf in _leaves(model):
        into = groups[1] if isinstance(leaf, _bn_types()) else groups[0]
        for p in leaf.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                into.append(p)
    return list(groups)


def group_names(model):
    """layer_groups as state-dict key names"""
    name = {id(p): k for k, p in model.named_parameters()}
    return [[name[id(p)] for p in g] for g in layer_groups(model)]


# ---------------------------------------------------------------------------------------------------------------------- chunk table
def chunks_of(numel, used):
    """The per-chunk columns of csrc/optim.hip's table: numel (T,) i64, used (T,) bool -> (chunk_tensor i32, chunk_start i64); every
    used tensor is cut into chunks of at most CHUNK consecutive elements, in tensor order"""
    counts = np.where(used, (numel + CHUNK - 1) // CHUNK, 0)
    first = np.cumsum(counts) - counts
    chunk_tensor = np.repeat(np.arange(len(numel), dtype=np.int32), counts)
    chunk_start = (np.arange(len(chunk_tensor), dtype=np.int64) - np.repeat(first, counts)) * CHUNK
    return chunk_tensor, chunk_start


def upload_sections(sections, device):
    """[(name, array)] -> (ONE device byte buffer holding every array at an 8-byte aligned offset, {name: device address}): one upload"""
    import torch
    blob, offset = [], {}
    at = 0
    for name, a in sections:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        pad = (-len(raw)) % 8
        offset[name] = at
        blob += [raw, np.zeros(pad, dtype=np.uint8)]
        at += len(raw) + pad
    buf = torch.from_numpy(np.concatenate(blob)).to(device)
    base = buf.data_ptr()
    return buf, {name: base + off for name, off in offset.items()}


# ------------------------------------------------------------------------------------------------------------------------ optimizer
class OneCycleAdam:
    def __init__(self, model, total_steps, lr_max, moms, div_factor, pct_start, wd, grad_norm_clip, betas2=0.99, eps=1e-8, device=None,
                 group=None):
        import torch
        self.model = model
        self.total_steps, self.lr_max, self.moms = int(total_steps), float(lr_max), [float(m) for m in moms]
        self.div_factor, self.pct_start = float(div_factor), float(pct_start)
        self.wd, self.grad_norm_clip, self.betas2, self.eps = float(wd), float(grad_norm_clip), float(betas2), float(eps)
        if not self.grad_norm_clip > 0:
            raise ValueError("optim: grad_norm_clip %r" % (grad_norm_clip,))
        self.groups = [[p for p in g if p.requires_grad] for g in layer_groups(model)]          # trainable_params at creation
        self.params = self.groups[0] + self.groups[1]
        if not self.params:
            raise ValueError("optim: the model has no trainable parameter")
        own = {id(p) for p in self.params}
        self._others = [p for p in model.parameters() if id(p) not in own]                       # clipped with the rest, never stepped
        self.device = torch.device(device) if device is not None else self.params[0].device
        self.group = group if group is not None and group.active else None                       # dist_train.ReplicaGroup: grads are summed over its ranks
        self._bucket, self._layout_checked, self.table_uploads = None, None, 0
        self._check()
        self.lr, self.mom = self.lr_max / self.div_factor, self.moms[0]
        self.steps_done = 0
        self.total_norm = None
        template = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=0, betas=(0.9, self.betas2), eps=self.eps).param_groups[0]
        self._group_keys = {k: v for k, v in template.items() if k != "params"}                 # the installed Adam's keys and defaults
        if self.device.type == "cpu":
            self._adam = torch.optim.Adam([{"params": g, "lr": 0} for g in self.groups], betas=(0.9, self.betas2), eps=self.eps, foreach=False)
        else:
            self.state = {}                                   # index -> {"step": int, "exp_avg", "exp_avg_sq"}
            self._signature, self._table, self._work, self._held = None, None, None, []

    # ------------------------------------------------------------------------------------------------------------------- interface
    def schedule(self, it):
        """lr_scheduler.step(it): the one-cycle lr and beta1 of iteration ``it``"""
        self.lr, self.mom = one_cycle(it, self.total_steps, self.lr_max, self.moms, self.div_factor, self.pct_start)

    def zero_grad(self):
        """torch's Optimizer.zero_grad(): the grads of the groups' parameters become None"""
        for p in self.params:
            p.grad = None

    def step(self):
        self._check()
        if self.device.type == "cpu":
            self._step_cpu()
        else:
            self._step_device()
        self.steps_done += 1

    def _check(self):
        import torch
        for p in self.params + self._others:
            if p.device != self.device:
                raise ValueError("optim: a parameter lives on %s, the optimizer on %s" % (p.device, self.device))
        for p in self.params:
            ok = p.dtype == torch.float32 or (self.device.type == "cpu" and p.dtype == torch.float64)
            if not ok or not p.is_contiguous():
                raise ValueError("optim: parameters must be contiguous float32 tensors (%s, strides %s)" % (p.dtype, tuple(p.stride())))
            if p.grad is not None and p.grad.dtype != p.dtype:
                raise ValueError("optim: a grad of dtype %s on a parameter of dtype %s" % (p.grad.dtype, p.dtype))

    # --------------------------------------------------------------------------------------------------------------------- checker
    def _sync_groups(self):
        for g in self._adam.param_groups:
            g["lr"], g["betas"], g["weight_decay"] = self.lr, (self.mom, self.betas2), 0

    def _step_cpu(self):
        from torch.nn.utils import clip_grad_norm_
        if self.group is not None:                           # the checker's exchange: every grad summed over the ranks, in place
            tensors = self.params + self._others
            self._check_layout(tensors, [p.grad for p in tensors])
            for p in tensors:
                if p.grad is not None:
                    self.group.all_reduce_bucket(p.grad)
        self.total_norm = clip_grad_norm_(self.params + self._others, self.grad_norm_clip)       # Trainer._train_it
        for g in self._adam.param_groups:                                                        # OptimWrapper.step, true_wd and bn_wd
            for p in g["params"]:
                if p.requires_grad is False:
                    continue
                p.data.mul_(1 - self.wd * self.lr)
        self._sync_groups()
        self._adam.step()

    # ---------------------------------------------------------------------------------------------------------------------- device
    def _grads(self):
        """-> the contiguous grad (or None) of every tensor of the table; a non-contiguous grad is copied"""
        out = []
        for p in self.params + self._others:
            g = p.grad
            if g is not None and (g.dtype != p.dtype or g.device != p.device):
                raise ValueError("optim: a grad of dtype %s on %s for a parameter of dtype %s on %s" % (g.dtype, g.device, p.dtype, p.device))
            out.append(g if g is None or g.is_contiguous() else g.contiguous())
        return out

    def _check_layout(self, tensors, grads):
        """With a group: the set of tensors that have a grad must be the same on every rank (the ranks exchange slots of one layout); its
        hash is all-gathered whenever it changes"""
        layout = tuple((i, p.numel()) for i, (p, g) in enumerate(zip(tensors, grads)) if g is not None)
        if layout != self._layout_checked:
            self.group.check_layout(layout)
            self._layout_checked = layout

    def _build_bucket(self, tensors, grads):
        """The flat f32 bucket of the tensors that have a grad (dist_train.bucket_layout; padding zeroed here and never written)
        -> (slot_start (T,) i64, the bucket)"""
        import torch
        from .dist_train import bucket_layout
        has = [i for i, g in enumerate(grads) if g is not None]
        starts, total = bucket_layout([tensors[i].numel() for i in has])
        slot_start = np.zeros(len(tensors), dtype=np.int64)
        slot_start[has] = starts
        if self._bucket is None or self._bucket.numel() != max(total, 1):
            self._bucket = torch.zeros((max(total, 1),), dtype=torch.float32, device=self.device)
        else:
            self._bucket.zero_()                              # another layout of the same size: what was a slot may now be padding
        return slot_start, self._bucket

    def _build_table(self, tensors, grads):
        """The chunk table of csrc/optim.hip as ONE device byte buffer (one upload): per tensor param / grad / exp_avg / exp_avg_sq
        addresses, numel, step, flags; per chunk tensor index and start.  -> dict of section addresses, n_tensors, n_chunks.
        With a group the grad column points into the bucket and two columns are added: src (the tensors' own grads) and slot_start."""
        import torch
        n_own = len(self.params)
        T = len(tensors)
        addr = np.zeros((4, T), dtype=np.uint64)
        numel = np.array([p.numel() for p in tensors], dtype=np.int64)
        extra = []
        if self.group is not None:
            slot_start, bucket = self._build_bucket(tensors, grads)
            src = np.array([0 if g is None else g.data_ptr() for g in grads], dtype=np.uint64)
            extra = [("src", src), ("slot_start", slot_start)]
            grads = [None if g is None else bucket[int(s):int(s) + g.numel()] for g, s in zip(grads, slot_start)]
        flags, steps = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.int32)
        for i, (p, g) in enumerate(zip(tensors, grads)):
            addr[0, i] = p.data_ptr()
            addr[1, i] = 0 if g is None else g.data_ptr()
            if i < n_own and p.requires_grad:
                flags[i] = FLAG_DECAY
                if g is not None:
                    st = self.state.get(i)
                    if st is None:                           # lazily, as Adam._init_group
                        st = self.state[i] = {"step": 0, "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                              "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
                    flags[i] |= FLAG_ADAM
                    addr[2, i], addr[3, i], steps[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"]
        used = (flags != 0) | (addr[1] != 0)
        chunk_tensor, chunk_start = chunks_of(numel, used)
        sections = [("param", addr[0]), ("grad", addr[1]), ("exp_avg", addr[2]), ("exp_avg_sq", addr[3]), ("numel", numel),
                    ("chunk_start", chunk_start)] + extra + [("steps", steps), ("chunk_tensor", chunk_tensor), ("flags", flags)]   # 8-byte columns first
        buf, at = upload_sections(sections, self.device)
        self.table_uploads += 1
        return {"buf": buf, "n_tensors": T, "n_chunks": int(len(chunk_tensor)), "adam": np.nonzero(flags & FLAG_ADAM)[0], **at}

    def _step_device(self):
        import torch
        tensors = self.params + self._others
        grads = self._grads()
        signature = tuple((p.data_ptr(), p.requires_grad, None if g is None else g.data_ptr()) for p, g in zip(tensors, grads))
        if signature != self._signature:
            if self.group is not None:
                self._check_layout(tensors, grads)
            self._table = self._build_table(tensors, grads)
            need = _lib.call("prcnn_optim_workspace", self._table["n_chunks"])
            if self._work is None or self._work.numel() < need:
                self._work = torch.zeros((need,), dtype=torch.float64, device=self.device)
            self.total_norm = self._work[0]
            self._signature = signature
        self._held = grads                                    # the copies of non-contiguous grads live until the next step
        t = self._table
        if t["n_chunks"] == 0:                                # nothing has a grad and nothing decays
            return
        stream = C.c_void_p(_lib.current_stream(self._work))
        nt, nc, work = t["n_tensors"], t["n_chunks"], self._work.data_ptr()
        if self.group is not None:                            # the table's grad column points into the bucket: pack, one exchange, then the step
            _lib.call("prcnn_grad_pack", t["src"], t["numel"], t["slot_start"], t["chunk_tensor"], t["chunk_start"], nt, nc,
                      self._bucket.data_ptr(), self._bucket.numel(), stream)
            self.group.all_reduce_bucket(self._bucket)
        _lib.call("prcnn_optim_sumsq", t["grad"], t["numel"], t["chunk_tensor"], t["chunk_start"], nt, nc, work, stream)
        _lib.call("prcnn_optim_finish", t["flags"], t["steps"], nt, nc, self.grad_norm_clip, work, stream)
        _lib.call("prcnn_optim_update", t["param"], t["grad"], t["exp_avg"], t["exp_avg_sq"], t["numel"], t["flags"], t["steps"], t["chunk_tensor"],
                  t["chunk_start"], nt, nc, self.lr, self.mom, self.betas2, self.eps, self.wd, work, stream)
        for i in t["adam"]:                                   # the host's mirror of the device's step column
            self.state[int(i)]["step"] += 1

    # ------------------------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        import torch
        if self.device.type == "cpu":
            self._sync_groups()
            return self._adam.state_dict()
        groups, at = [], 0
        for g in self.groups:
            groups.append(dict(self._group_keys, lr=self.lr, betas=(self.mom, self.betas2), weight_decay=0, params=list(range(at, at + len(g)))))
            at += len(g)
        state = {i: {"step": torch.tensor(float(st["step"]), dtype=torch.float32), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
                 for i, st in sorted(self.state.items())}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        import torch
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != [len(g) for g in self.groups]:
            raise ValueError("optim: the checkpoint's groups hold %s parameters, this model's %s" %
                             ([len(g["params"]) for g in groups], [len(g) for g in self.groups]))
        self.lr, self.mom = float(groups[0]["lr"]), float(groups[0]["betas"][0])
        steps = [int(float(st["step"])) for st in sd["state"].values()]
        self.steps_done = max(steps, default=0)
        if self.device.type == "cpu":
            self._adam.load_state_dict(sd)
            for g in self._adam.param_groups:
                g["foreach"] = False
            return
        index = [i for g in groups for i in g["params"]]      # the checkpoint's ids in group order -> positions 0 .. n - 1
        where = {pid: k for k, pid in enumerate(index)}
        self.state = {}
        for pid, st in sd["state"].items():
            k = where[pid]
            p = self.params[k]
            conv = lambda v: v.detach().to(device=self.device, dtype=torch.float32).reshape(p.shape).contiguous().clone()
            self.state[k] = {"step": int(float(st["step"])), "exp_avg": conv(st["exp_avg"]), "exp_avg_sq": conv(st["exp_avg_sq"])}
        self._signature = None                                # the table is rebuilt (and the step column uploaded) by the next step
