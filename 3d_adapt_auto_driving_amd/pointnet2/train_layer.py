"""The order-fixed training layer: forward and backward of a ``pytorch_utils`` conv block -- 1x1 convolution, BatchNorm on batch
statistics, ReLU -- on the project's own gfx950 kernels (csrc/train_layer.hip; include/prcnn_hip.h states the arithmetic contract;
DESIGN.md section 29).  Sums have a fixed shape and there are no float atomics: the same input gives the same bits.

Selected by ``pytorch_utils.FUSED_TRAIN_LAYERS`` (off by default; ``pytorch_utils.fused_train_layers()``).  ``covers(block, x)`` says
which blocks it serves; every other block runs its ``nn.Sequential`` forward exactly as before.  An extension module without the
entries (the compiled dropin_native modules export the reference's nine names) RAISES by name: torch's modules are never taken in
its place once the switch is on and the block is covered.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import pointnet2_utils


def _entry(name):
    ext = pointnet2_utils.pointnet2
    fn = getattr(ext, name, None)
    if fn is None:
        raise RuntimeError("fused training layers are selected but extension module %s has no entry %r (torch's modules are never "
                           "taken in its place)" % (getattr(ext, "__name__", ext), name))
    return fn


class TrainLayer(Function):
    """y = act(bn(conv1x1(x))).  gamma None: no BatchNorm, beta is then the convolution's bias (or None).  The running buffers are
    updated in place by the forward.  Returns a new tensor (the block's in-place ReLU is not emulated)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.contiguous()
        w = w.contiguous()
        y, z, stats = _entry("train_layer_forward_wrapper")(x, w, gamma, beta, eps, momentum, running_mean, running_var, relu)
        ctx.relu = bool(relu)
        ctx.stats = stats                         # (2, cout) f64: mean, rstd
        if gamma is not None:
            ctx.save_for_backward(x, w, z, gamma, beta)
        else:
            ctx.save_for_backward(x, w, y if relu else None, None, None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, zy, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad
        bn = gamma is not None
        dx, dw, dgamma, dbeta = _entry("train_layer_backward_wrapper")(dy.contiguous(), x, w, zy, gamma, beta, ctx.stats, ctx.relu,
                                                                       need[0], need[1], bn or need[3])
        return (dx, dw, dgamma if need[2] else None, dbeta if need[3] else None, None, None, None, None, None)


def _parts(block):
    """-> (conv, bn module or None, activation or None), or None for a block of another build"""
    names = [k for k, _ in block.named_children()]
    mods = dict(block.named_children())
    if not names or names[0] != "conv" or any(k not in ("conv", "bn", "activation") for k in names):
        return None                               # preact (the convolution is not first), instance norm, a name prefix
    bn = mods.get("bn")
    if bn is not None:
        bn = bn[0] if isinstance(bn, nn.Sequential) and len(bn) == 1 else None
        if not isinstance(bn, (nn.BatchNorm1d, nn.BatchNorm2d)):
            return None
    return mods["conv"], bn, mods.get("activation")


def covers(block, x):
    """Does the fused layer serve this block on this input?  A 1x1 convolution first (post-activation order), then BatchNorm or
    none, then nn.ReLU or none; no instance norm; bn.momentum a float; training mode; a CUDA f32 input."""
    if not block.training or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 3 or x.numel() == 0:
        return False
    parts = _parts(block)
    if parts is None:
        return False
    conv, bn, act = parts
    if not isinstance(conv, (nn.Conv1d, nn.Conv2d)) or x.dim() != (3 if isinstance(conv, nn.Conv1d) else 4):
        return False
    one = lambda v, k: all(int(e) == k for e in (v if isinstance(v, (tuple, list)) else (v,)))
    if not (one(conv.kernel_size, 1) and one(conv.stride, 1) and one(conv.padding, 0) and one(conv.dilation, 1) and conv.groups == 1):
        return False
    if conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    if act is not None and type(act) is not nn.ReLU:
        return False
    if bn is not None:
        if conv.bias is not None or not bn.affine or not bn.track_running_stats or not isinstance(bn.momentum, float) or not bn.training:
            return False
    return True


def run(block, x):
    """The block's forward through TrainLayer (covers(block, x) holds)"""
    conv, bn, act = _parts(block)
    relu = act is not None
    if bn is None:
        return TrainLayer.apply(x, conv.weight, None, conv.bias, None, None, 0.0, 0.0, relu)
    if x.numel() // x.shape[1] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    y = TrainLayer.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu)
    bn.num_batches_tracked.add_(1)
    return y
