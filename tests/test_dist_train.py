"""Data-parallel training on the CPU (dist_train.py, optim.OneCycleAdam(group=...), train_rcnn under a launcher's variables) over gloo
worlds of spawned processes.  The comparisons are BIT FOR BIT: at a world of 2 the reduced gradient is a two-term f32 sum (commutative),
at a world of 4 the inputs are lattice numbers whose every sum is exact; tests/dist_replica.py holds the single-process definition."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dist_replica as DR  # noqa: E402
import optim_batch as OB  # noqa: E402

PKG = DR.PKG


@pytest.fixture(autouse=True)
def one_thread():
    """One thread here as in the workers (the reference and the ranks must sum in the same order); the suite's own count comes back"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------------ layout, shard
def test_bucket_layout_slots_are_aligned_disjoint_and_in_order():
    D = DR.D()
    numels = [1, 63, 64, 65, 0, 2047, 2048, 2049, 3 * 2048 + 5]
    starts, total = D.bucket_layout(numels)
    assert D.ALIGN == 64 and len(starts) == len(numels)
    assert all(s % 64 == 0 for s in starts) and total % 64 == 0
    for k in range(len(numels) - 1):
        assert starts[k] + numels[k] <= starts[k + 1]                            # disjoint, in table order
        assert starts[k + 1] - starts[k] == -(-numels[k] // 64) * 64             # no gap beyond the padding
    assert starts[0] == 0 and starts[-1] + numels[-1] <= total < starts[-1] + numels[-1] + 64
    assert D.bucket_layout([]) == ([], 0)
    with pytest.raises(ValueError):
        D.bucket_layout([3, -1])


def test_shard_is_the_contiguous_scatter_chunk_and_a_world_of_one_is_the_identity(monkeypatch):
    D = DR.D()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    import torch.distributed as dist
    g = D.ReplicaGroup.from_env("cpu")
    assert (g.rank, g.world, g.active, g.backend) == (0, 1, False, "gloo") and not dist.is_initialized()
    idx = np.arange(12)
    assert g.shard(idx) is idx
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not D.ReplicaGroup.from_env("cpu").active and not dist.is_initialized()
    # the arithmetic of shard() needs no process group: a group object without one
    for W in (2, 3, 4):
        parts = []
        for r in range(W):
            h = object.__new__(D.ReplicaGroup)
            h.rank, h.world = r, W
            parts.append(h.shard(idx))
            assert list(parts[-1]) == list(range(r * 12 // W, (r + 1) * 12 // W))
        assert list(np.concatenate(parts)) == list(idx)
    h = object.__new__(D.ReplicaGroup)
    h.rank, h.world = 0, 5
    with pytest.raises(ValueError, match="does not divide"):
        h.shard(idx)
    rows = {"a": torch.ones(3, 2)}
    assert g.gather_rows(rows)["a"] is rows["a"] and g.all_reduce_bucket(rows["a"]) is rows["a"]
    assert D.default_backend("cuda") == "nccl" and D.default_backend("cpu") == "gloo"


# --------------------------------------------------------------------------------------------------------------------- definition
def test_replica_reference_keeps_shard_zeros_batchnorm_update_and_accumulates_both_shards():
    cfg = DR.small_cfg("DiceLoss")
    batch = DR.small_batch(cfg, 2)
    model = DR.small_model(cfg)
    out = DR.replica_reference(model, DR.small_forward, DR.small_loss_fn(cfg), batch, 2)
    assert out[2]["parts"].shape[0] > 0 and np.isfinite(float(out[0].detach()))
    alone = DR.small_model(cfg)                                                   # shard 0 alone: the same BatchNorm buffers
    DR.small_forward(alone, DR.shard_of(batch, 0, 2))
    assert torch.equal(alone.bn.running_mean, model.bn.running_mean) and torch.equal(alone.bn.running_var, model.bn.running_var)
    assert int(model.bn.num_batches_tracked) == 1
    other = DR.small_model(cfg)
    DR.small_forward(other, DR.shard_of(batch, 1, 2))
    assert not torch.equal(other.bn.running_mean, model.bn.running_mean)
    assert all(p.grad is not None for p in model.parameters())
    whole = DR.small_model(cfg)                                                   # NOT the whole batch through one BatchNorm
    res = DR.small_loss_fn(cfg)(DR.small_forward(whole, batch))
    assert float(res[0].detach()) != float(out[0].detach())


# ------------------------------------------------------------------------------------------------------------------------ world 2
@pytest.fixture(scope="module")
def world2():
    return DR.run_world(DR.world2_iterations, 2)


@pytest.mark.parametrize("kind", DR.KINDS)
def test_world2_iteration_equals_the_definition_bit_for_bit(world2, kind):
    want = DR.reference_iteration(kind, 2)
    for rank in range(2):
        got = world2[rank][kind]
        assert got["grads_none"] == [] and got["reg_grad_is_zero"] == (rank == 1)          # zero, not None: the layouts agree
        assert DR.same_snapshot(want, {k: v for k, v in got.items() if k != "reg_grad_is_zero"}) == [], (kind, rank)
        assert got["tb_dict"] == want["tb_dict"] and got["tb_dict"]["rpn_fg_sum"] > 0
    r0, r1 = world2[0][kind]["buffers"], world2[1][kind]["buffers"]
    for k in want["buffers"]:
        assert r0[k].tobytes() == want["buffers"][k].tobytes(), k                            # rank 0's buffers are the checkpoint's
    assert r0["bn.running_mean"].tobytes() != r1["bn.running_mean"].tobytes()                # statistics are per replica
    assert want["total_norm"] > 0 and len(want["exp_avg"]) == 8


def test_world2_drift_raises_on_every_rank(world2):
    for rank in range(2):
        d = world2[rank]["drift"]
        assert d["agreed"] == world2[0]["drift"]["agreed"]
        assert d["raised"] is not None and "replica drift" in d["raised"], (rank, d)


# ------------------------------------------------------------------------------------------------------------------------ world 4
def test_world4_optimizer_step_equals_one_step_on_the_summed_gradients():
    got = DR.run_world(DR.world4_step, 4)
    model = OB.tiny_model()
    names, sizes = OB.layout(model)
    total = int(sum(sizes))
    parts = [DR.lattice_grads(total, r) for r in range(4)]
    summed = (parts[0] + parts[1]) + (parts[2] + parts[3])
    assert np.array_equal(summed.astype(np.float64), sum(p.astype(np.float64) for p in parts))   # every 4-term sum is exact
    opt = OB.O().OneCycleAdam(model, **OB.HYPER)
    OB.freeze(model)
    opt.schedule(0)
    OB.set_grads(model, names, summed, sizes)
    opt.step()
    want = DR.snapshot(model, opt, None)
    assert want["total_norm"] > 1.0 and len(want["exp_avg"]) > 0
    for rank in range(4):
        assert DR.same_snapshot(want, got[rank], skip=("buffers", "grads_none")) == [], rank


def test_a_rank_without_a_grad_the_others_have_raises_by_name():
    got = DR.run_world(DR.layout_mismatch, 2)
    assert all(m is not None and "bucket layout mismatch" in m for m in got), got


# ------------------------------------------------------------------------------------------------------------------------- digest
def test_host_digest_equals_its_definition():
    D = DR.D()
    rng = np.random.RandomState(3)
    sizes = [1, 63, 64, 65, 200]
    arrays = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    starts, _ = D.bucket_layout(sizes)
    want = 0
    for a, s in zip(arrays, starts):                                              # the definition, in Python integers
        for j, bits in enumerate(a.view(np.uint32).tolist()):
            want = (want + bits * (2 * (s + j) + 1)) % (1 << 64)
    assert D.host_digest(arrays) == want and want != 0
    assert D.digest([torch.from_numpy(a) for a in arrays]) == want
    flipped = [a.copy() for a in arrays]
    flipped[-1].view(np.uint32)[-1] ^= 1                                          # one mantissa bit of the last element
    assert D.host_digest(flipped) != want


# ------------------------------------------------------------------------------------------------------------------- command line
def test_train_rcnn_refuses_a_batch_that_does_not_divide_over_the_world(tmp_path, monkeypatch):
    import importlib
    T = importlib.import_module(PKG + ".train_rcnn")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="batch_size 3"):
        T.main(["--train_mode", "rpn", "--root", str(tmp_path / "no_tree"), "--batch_size", "3", "--device", "cpu", "--output_dir", str(out)])
    assert not out.exists() and list(tmp_path.iterdir()) == []
    with pytest.raises(NotImplementedError, match="--mgpus"):
        T.main(["--train_mode", "rpn", "--root", str(tmp_path), "--mgpus", "--output_dir", str(out)])
    assert not out.exists()
