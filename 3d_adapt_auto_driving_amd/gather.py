"""Scene sharding across ranks and the ONE collective of the job: the all-gather of the padded detection tables."""
import numpy as np
import torch


def shard_scene_ids(num_scenes, rank, world):
    """Rank r evaluates scenes r, r+world, ... (independent units)."""
    return list(range(rank, num_scenes, world))


def pack_detections(scene_ids, det_batches, max_det):
    """Host-side table [S, max_det, 9] = 7 box + score + scene id, zero padded, plus counts [S].
    numpy on purpose: the per-batch slice assignments of the first version were torch CPU kernels, each of which may fan out
    over the host's OpenMP pool -- tens of milliseconds for 20 batches on a 128-core box, inside the bench's clock."""
    S = len(scene_ids)
    table = np.empty((S, max_det, 9), dtype=np.float32)
    det_batches = list(det_batches)
    if det_batches:
        table[:, :, 0:7] = np.concatenate([np.asarray(d[0]) for d in det_batches], 0)
        table[:, :, 7] = np.concatenate([np.asarray(d[1]) for d in det_batches], 0)
        counts = np.concatenate([np.asarray(d[2]) for d in det_batches], 0).astype(np.int32)
    else:
        counts = np.zeros((0,), dtype=np.int32)
    table[:, :, 8] = np.asarray(scene_ids, dtype=np.float32).reshape(-1, 1)
    return torch.from_numpy(table), torch.from_numpy(counts)


def all_gather_detections(table, counts, device, force=False):
    """The ONE collective of the job: all ranks exchange their padded detection tables
    (RCCL all_gather over xGMI when the backend is nccl; gloo in the CPU tests).  Tables are
    padded to the largest per-rank scene count so that all_gather_into_tensor applies; the padding rows
    (count -1) are stripped and the rows come back in scene-id order on every rank.
    ``force``: run the exchange on a world of ONE rank as well (the identity up to the id sort) instead of returning early -- how
    the RCCL leg (device-side padding, both all_gather_into_tensor calls on HIP tensors, strip, sort) is exercised on a 1-GPU box
    (tests/test_gpu_configs.py; bench.py --gpus 1 under torchrun sets it when PRCNN_FORCE_GATHER=1)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        if force:
            raise RuntimeError("all_gather_detections(force=True): torch.distributed is not initialised")
        return table, counts
    if dist.get_world_size() == 1 and not force:
        return table, counts
    world = dist.get_world_size()
    n_local = torch.tensor([table.shape[0]], dtype=torch.int64, device=device)
    sizes = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(sizes, n_local)
    smax = int(max(int(s.item()) for s in sizes))
    pad_t = torch.zeros((smax,) + tuple(table.shape[1:]), dtype=table.dtype, device=device)
    pad_c = torch.full((smax,), -1, dtype=torch.int32, device=device)   # -1 marks padding rows
    pad_t[:table.shape[0]] = table.to(device)
    pad_c[:counts.shape[0]] = counts.to(device)
    out_t = torch.empty((world * smax,) + tuple(table.shape[1:]), dtype=table.dtype, device=device)
    out_c = torch.empty((world * smax,), dtype=torch.int32, device=device)
    dist.all_gather_into_tensor(out_t, pad_t)
    dist.all_gather_into_tensor(out_c, pad_c)
    real = out_c >= 0
    out_t, out_c = out_t[real].cpu(), out_c[real].cpu()
    # rank-major as gathered (r, r + W, ... per rank) -> scene-id order, the order of a single-process run: what rank 0 writes and
    # scores does not depend on the world size (ids are exact in float32 up to 2^24 scenes)
    order = torch.argsort(out_t[:, 0, 8], stable=True) if out_t.shape[0] and out_t.shape[1] else torch.arange(out_t.shape[0])
    return out_t[order].contiguous(), out_c[order].contiguous()
