"""Data-parallel training: one process per GPU, nn.DataParallel's semantics (the reference's --mgpus) in the shape the eval driver has.

  group = ReplicaGroup.from_env(device, backend)        # RANK / WORLD_SIZE / LOCAL_RANK as a launcher (torchrun) sets them
  rows  = group.shard(perm[k B:(k + 1) B])              # rank r's contiguous b = B / W rows of the GLOBAL batch
  loss, tb_dict, disp_dict = model_fn_replicas(cfg, model, src.batch(rows), group);  loss.backward()
  OneCycleAdam(model, ..., group=group).step()          # pack -> ONE all-reduce of the flat bucket -> the three launches of the step
  group.digest_check(model.parameters())                # before a checkpoint: replicas that drifted raise instead of saving

What a W-rank iteration computes: every rank runs the forward on its own rows in training mode (BatchNorm batch statistics are per
replica); the rows the loss reads (losses.RPN_ROWS / RCNN_ROWS) are gathered over the ranks in rank order by ONE autograd function whose
backward hands each rank its slice of the incoming gradient (no reduce-scatter: every rank evaluates the same whole-batch loss); the loss
runs unchanged on the gathered rows, so every normalizer and Dice's ratio of sums are the whole batch's and tb_dict is identical on every
rank; parameter gradients are SUMMED over the ranks (the loss is already the whole batch's), the clip norm is taken of the sum and every
rank applies the same step.  At W = 2 the sum has two f32 terms and is what one process gets by accumulating both shards' gradients, bit
for bit; for W > 2 it equals that sum up to the order of W terms.

The exchange of a CUDA model (csrc/grad_bucket.hip): prcnn_grad_pack copies every gradient into one flat f32 bucket in one launch over the
optimizer's chunk table, the bucket is all-reduced once, and the table's grad column points into the bucket, so the step reads the reduced
gradients there and ``p.grad`` stays the rank's own.  bucket_layout() is the layout: slots in table order, each at a multiple of 64
elements, padding zeroed at allocation and never written; only tensors that have a grad get a slot, and that set must be the same on every
rank (check_layout: a hash of it is all-gathered whenever it changes; a mismatch raises).  prcnn_param_digest is the drift check's
64-bit digest, sum of bits(p[i]) (2 i + 1) mod 2^64 with i the element's index in bucket_layout() of ALL the tensors given.

Backends: "nccl" (RCCL; the default for CUDA) exchanges device tensors; "gloo" (the default for cpu) exchanges host tensors, and with
device tensors this module stages every exchange buffer through a host copy itself -- that is also how two ranks can share one GPU in the
tests.  A world of 1 creates no process group and every method is the identity, unless ``force`` routes the exchanges through the backend
anyway (tests and profiles/dist_exchange_probe.py).
"""
import hashlib
import os

import numpy as np

from . import _lib, losses
from .optim import chunks_of, upload_sections

ALIGN = _lib.PRCNN_BUCKET_ALIGN
_M64 = (1 << 64) - 1


# --------------------------------------------------------------------------------------------------------------------------- layout
def bucket_layout(numels):
    """-> (slot_start list, total): slots in the order given, each starting at a multiple of ALIGN elements; total is a multiple too"""
    starts, at = [], 0
    for n in numels:
        n = int(n)
        if n < 0:
            raise ValueError("bucket_layout: a tensor of %d elements" % n)
        starts.append(at)
        at += -(-n // ALIGN) * ALIGN
    return starts, at


def layout_hash(layout):
    """63 bits of a hash of the layout signature ((table index, numel) of every tensor that has a grad)"""
    return int.from_bytes(hashlib.sha256(repr(tuple(layout)).encode()).digest()[:8], "little") >> 1


def host_digest(arrays):
    """The digest's definition on host arrays of 32-bit elements: sum of bits(p[i]) (2 i + 1) mod 2^64, i the element's index in
    bucket_layout of the arrays' sizes"""
    starts, _total = bucket_layout([a.size for a in arrays])
    total = 0
    for a, s in zip(arrays, starts):
        bits = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
        k = np.arange(s, s + bits.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        total = (total + int((bits * k).sum(dtype=np.uint64))) & _M64          # (uint64 arithmetic wraps: that is the mod)
    return total


def device_digest(tensors):
    """prcnn_param_digest of contiguous f32 CUDA tensors -> int (one read of 8 bytes)"""
    import ctypes as C
    import torch
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("dist_train: the digest takes contiguous float32 CUDA tensors (%s, %s)" % (t.dtype, t.device))
    numel = np.array([t.numel() for t in tensors], dtype=np.int64)
    starts, _total = bucket_layout(numel)
    chunk_tensor, chunk_start = chunks_of(numel, numel > 0)
    if len(chunk_tensor) == 0:
        return 0
    dev = tensors[0].device
    addr = np.array([t.data_ptr() for t in tensors], dtype=np.uint64)
    buf, at = upload_sections([("param", addr), ("numel", numel), ("slot_start", np.array(starts, dtype=np.int64)),
                               ("chunk_start", chunk_start), ("chunk_tensor", chunk_tensor)], dev)
    work = torch.zeros((1 + len(chunk_tensor),), dtype=torch.int64, device=dev)
    _lib.call("prcnn_param_digest", at["param"], at["numel"], at["slot_start"], at["chunk_tensor"], at["chunk_start"], len(tensors),
              len(chunk_tensor), work.data_ptr(), C.c_void_p(_lib.current_stream(work)))
    out = int(work[0].item()) & _M64
    del buf
    return out


def digest(tensors):
    """The 64-bit digest of a list of f32 tensors, on the path their device selects"""
    tensors = [t.detach() for t in tensors]
    if tensors and tensors[0].is_cuda:
        return device_digest(tensors)
    return host_digest([t.contiguous().numpy() for t in tensors])


# ---------------------------------------------------------------------------------------------------------------------------- group
def world_from_env(environ=None):
    """-> (rank, world, local_rank) as a launcher sets them; (0, 1, 0) without"""
    e = os.environ if environ is None else environ
    world = int(e.get("WORLD_SIZE", "1") or 1)
    if world <= 1:
        return 0, 1, int(e.get("LOCAL_RANK", "0") or 0)
    if "RANK" not in e:
        raise ValueError("dist_train: WORLD_SIZE=%d without RANK (start the ranks under a launcher such as torchrun)" % world)
    return int(e["RANK"]), world, int(e.get("LOCAL_RANK", e["RANK"]))


def default_backend(device):
    return "gloo" if str(device).startswith("cpu") else "nccl"


_GatherRows = None


def _gather_function():
    import torch

    class GatherRows(torch.autograd.Function):
        """(group, *tensors) -> every tensor's rows of all ranks, concatenated in rank order; backward: this rank's slice"""
        @staticmethod
        def forward(ctx, group, *tensors):
            ctx.group, ctx.rows = group, [t.shape[0] for t in tensors]
            out = tuple(group.all_gather_rows(t.detach()) for t in tensors)
            ctx.mark_non_differentiable(*[o for o, t in zip(out, tensors) if not t.is_floating_point()])
            return out

        @staticmethod
        def backward(ctx, *grads):
            r = ctx.group.rank
            return (None,) + tuple(None if g is None else g[r * n:(r + 1) * n] for g, n in zip(grads, ctx.rows))
    return GatherRows


class ReplicaGroup:
    """The ranks of one data-parallel run.  ``active`` is False at a world of 1 (nothing is exchanged) unless ``force``."""

    def __init__(self, rank=0, world=1, device="cpu", backend=None, force=False):
        import torch
        self.rank, self.world = int(rank), int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError("dist_train: rank %d of a world of %d" % (self.rank, self.world))
        self.device = torch.device(device)
        self.backend = backend or default_backend(self.device)
        if self.backend not in ("nccl", "gloo"):
            raise ValueError("dist_train: --dist_backend %r (nccl or gloo)" % (self.backend,))
        self.active = self.world > 1 or bool(force)
        self.owns_process_group = False
        if self.active:
            import torch.distributed as dist
            if not dist.is_initialized():
                kw = {"device_id": self.device} if self.backend == "nccl" else {}
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world, **kw)
                self.owns_process_group = True
            if dist.get_world_size() != self.world or dist.get_rank() != self.rank:
                raise ValueError("dist_train: the process group is rank %d of %d, the ReplicaGroup rank %d of %d" %
                                 (dist.get_rank(), dist.get_world_size(), self.rank, self.world))

    @classmethod
    def from_env(cls, device="cuda", backend=None, environ=None):
        """The group a launcher's variables describe; ``device`` 'cuda' becomes cuda:LOCAL_RANK (and the current device)"""
        import torch
        rank, world, local = world_from_env(environ)
        dev = torch.device(device)
        if dev.type == "cuda" and world > 1:
            dev = torch.device("cuda", local if dev.index is None else dev.index)
            torch.cuda.set_device(dev)
        return cls(rank, world, dev, backend)

    def close(self):
        if self.owns_process_group:
            import torch.distributed as dist
            dist.destroy_process_group()
            self.owns_process_group = False

    # ------------------------------------------------------------------------------------------------------------------- sharding
    def shard(self, indices):
        """Rank r's rows [r b, (r + 1) b) of one global batch, b = len / world: DataParallel's contiguous scatter chunks"""
        n = len(indices)
        if n % self.world:
            raise ValueError("dist_train: a batch of %d does not divide over a world of %d" % (n, self.world))
        if self.world == 1:
            return indices
        b = n // self.world
        return indices[self.rank * b:(self.rank + 1) * b]

    # ------------------------------------------------------------------------------------------------------------------ exchanges
    def _staged(self, t):
        """Does this tensor go through a host copy?  gloo is given host tensors only"""
        return self.backend == "gloo" and t.is_cuda

    def all_gather_rows(self, t):
        """(n, ...) -> (world n, ...): the ranks' tensors concatenated along the first dimension in rank order (no autograd)"""
        import torch
        import torch.distributed as dist
        if not self.active:
            return t
        src = t.cpu() if self._staged(t) else t
        src = src.contiguous()
        out = torch.empty((self.world * src.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        dist.all_gather_into_tensor(out, src)
        return out.to(t.device) if self._staged(t) else out

    def gather_rows(self, rows):
        """{name: tensor} -> {name: the whole batch's rows}; ONE autograd function over all of them"""
        global _GatherRows
        if not self.active:
            return dict(rows)
        if _GatherRows is None:
            _GatherRows = _gather_function()
        keys = list(rows)
        return dict(zip(keys, _GatherRows.apply(self, *[rows[k] for k in keys])))

    def all_reduce_bucket(self, bucket):
        """In place: the sum of the ranks' buckets"""
        import torch.distributed as dist
        if not self.active:
            return bucket
        if self._staged(bucket) or not bucket.is_contiguous():
            host = bucket.cpu().contiguous() if self._staged(bucket) else bucket.contiguous()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            bucket.copy_(host)
        else:
            dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
        return bucket

    def all_gather_int(self, value):
        """One 64-bit value per rank -> the list of all ranks' values"""
        import torch
        if not self.active:
            return [int(value) & _M64]
        v = int(value) & _M64
        mine = torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64, device=self.device)
        return [int(x) & _M64 for x in self.all_gather_rows(mine).tolist()]

    def check_layout(self, layout):
        """Raises unless every rank's set of tensors with a grad is this one"""
        got = self.all_gather_int(layout_hash(layout))
        if len(set(got)) != 1:
            raise RuntimeError("dist_train: bucket layout mismatch: the set of tensors that have a gradient differs between the ranks "
                               "(rank %d: %d tensors, %d elements; hashes %s)" %
                               (self.rank, len(layout), sum(n for _i, n in layout), ["%016x" % h for h in got]))

    def digest_check(self, tensors):
        """All-gathers the parameters' digest; raises on EVERY rank if the replicas differ.  -> the digest"""
        mine = digest(list(tensors))
        got = self.all_gather_int(mine)
        if len(set(got)) != 1:
            raise RuntimeError("dist_train: replica drift: the ranks' parameter digests differ (%s)" % ["%016x" % h for h in got])
        return mine

    def broadcast_object(self, obj):
        """Rank 0's picklable ``obj`` to every rank (small host-side things: a sample list); the other ranks' argument is unread"""
        import torch.distributed as dist
        if not self.active:
            return obj
        box = [obj if self.rank == 0 else None]
        dist.broadcast_object_list(box, src=0, device=None if self.backend == "gloo" else self.device)
        return box[0]

    def broadcast_model(self, model):
        """Rank 0's parameters and buffers to every rank (once, after the checkpoints are loaded)"""
        import torch
        import torch.distributed as dist
        if not self.active:
            return
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                if self._staged(t) or not t.is_contiguous():
                    host = t.detach().cpu().contiguous() if self._staged(t) else t.detach().contiguous()
                    dist.broadcast(host, src=0)
                    t.copy_(host)
                else:
                    dist.broadcast(t.detach(), src=0)


# ------------------------------------------------------------------------------------------------------------------------- model_fn
def model_fn_replicas(cfg, model, shard_batch, group, forward=None, loss_fn=None):
    """losses.model_fn with the gather between the forward and the loss.  ``forward(model, shard_batch)`` -> the dictionary of rows the
    loss reads, ``loss_fn(rows)`` -> (loss, tb_dict, disp_dict); by default losses.forward_rows and losses.loss_of_rows under ``cfg``."""
    if forward is None:
        forward = lambda m, d: losses.forward_rows(cfg, m, d)
    if loss_fn is None:
        loss_fn = lambda rows: losses.loss_of_rows(cfg, rows)
    return loss_fn(group.gather_rows(forward(model, shard_batch)))
