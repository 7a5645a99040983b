"""world_size-2 and world_size-8 CPU tests (gloo) of the multi-GPU path: scene sharding + the single all_gather of
padded detection tables (eval_rcnn.shard_scene_ids / pack_detections / all_gather_detections).
The same code runs over RCCL (backend "nccl") on the GPU node; only the backend string differs."""
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_scenes, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from conftest import pkg
        from test_host_logic import tiny_model
        from oracle import ext_cpu, oracle as O
        O.set_num_threads(2)
        E = pkg("eval_rcnn")
        model, cfg, _ = tiny_model()
        ids = E.shard_scene_ids(n_scenes, rank, world)
        with ext_cpu.patch_package():
            table, counts = E.eval_synthetic(model, cfg, "cpu", ids, batch_size=2, npoints=2048)
        table, counts = E.all_gather_detections(table, counts, torch.device("cpu"))
        if rank == 0:
            np.savez(os.path.join(out_dir, "gathered.npz"), table=table.numpy(), counts=counts.numpy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_eval_all_gather_equals_single_process(tmp_path, oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import pkg
    from test_host_logic import tiny_model
    from oracle import ext_cpu
    E = pkg("eval_rcnn")
    n_scenes = 5                                   # odd: ranks get 3 and 2 scenes -> padded gather
    assert E.shard_scene_ids(5, 0, 2) == [0, 2, 4] and E.shard_scene_ids(5, 1, 2) == [1, 3]
    mp.spawn(_worker, args=(2, _free_port(), n_scenes, str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "gathered.npz")
    model, cfg, _ = tiny_model()
    with ext_cpu.patch_package():
        table, counts = E.eval_synthetic(model, cfg, "cpu", list(range(n_scenes)), batch_size=2, npoints=2048)
    # the gathered table lists rank 0's scenes then rank 1's: sort both by scene id (column 8)
    order = np.argsort(got["table"][:, 0, 8], kind="stable")
    assert got["table"].shape == (n_scenes, cfg.TEST.RPN_POST_NMS_TOP_N, 9)
    assert np.array_equal(got["table"][order][:, 0, 8], np.arange(n_scenes))
    assert np.array_equal(got["counts"][order], counts.numpy())
    np.testing.assert_allclose(got["table"][order], table.numpy(), rtol=0, atol=1e-6)
    assert counts.sum() > 0


def _scene_table(ids, max_det=100):
    """A detection table that regenerates from the scene ids alone (no model): box k of scene s = s + k / 128 + column / 1024,
    score = 1 / (1 + k), count = s % (max_det + 1) -- enough to tell any misplaced, duplicated or truncated row."""
    ids = np.asarray(ids, dtype=np.int64)
    k = np.arange(max_det, dtype=np.float32)[None, :, None]
    col = np.arange(7, dtype=np.float32)[None, None, :]
    table = np.zeros((len(ids), max_det, 9), np.float32)
    table[:, :, 0:7] = ids[:, None, None].astype(np.float32) + k / 128 + col / 1024
    table[:, :, 7] = 1.0 / (1.0 + k[:, :, 0])
    table[:, :, 8] = ids[:, None].astype(np.float32)
    counts = (ids % (max_det + 1)).astype(np.int32)
    return torch.from_numpy(table), torch.from_numpy(counts)


def _gather8_worker(rank, world, port, n_scenes, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.set_num_threads(1)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from conftest import pkg
        E = pkg("eval_rcnn")
        mine = E.shard_scene_ids(n_scenes, rank, world)
        table, counts = _scene_table(mine)
        t, c = E.all_gather_detections(table, counts, torch.device("cpu"))
        want_t, want_c = _scene_table(np.arange(n_scenes))
        ok = (tuple(t.shape) == (n_scenes, 100, 9) and torch.equal(t, want_t) and torch.equal(c, want_c) and c.dtype == torch.int32)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, len(mine), bool(ok), tuple(t.shape)))
    except Exception:
        q.put((rank, -1, "ERR " + traceback.format_exc(), None))


def test_world8_gather_of_the_kitti_val_split():
    """BASELINE configs[3] at its real shard sizes, without a model: 3769 scenes (split/kitti/val.txt) over 8 ranks = 472 on ranks
    0 .. 0 and 471 on the rest (r, r + 8, ...: pointrcnn/tools/batch_inference.py:95-107's split), one padded all_gather of
    (472, 100, 9) tables -- EVERY rank ends up with all 3769 rows, each exactly once, in scene-id order, the -1 padding rows of
    the seven shorter ranks stripped, counts int32."""
    from conftest import pkg
    E = pkg("eval_rcnn")
    n, world = 3769, 8
    sizes = [len(E.shard_scene_ids(n, r, world)) for r in range(world)]
    assert sizes == [472] + [471] * 7 and sum(sizes) == n
    assert sorted(i for r in range(world) for i in E.shard_scene_ids(n, r, world)) == list(range(n))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather8_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(60)
    for rank, n_mine, ok, shape in res:
        assert ok is True, (rank, ok, shape)
        assert n_mine == sizes[rank]


@pytest.mark.parametrize("ncores", [256, 128, 64])
def test_host_budget_world8_slices(ncores):
    """8 local ranks on a 256- / 128- / 64-core host: disjoint contiguous slices that cover the node, enqueue thread + loaders +
    writers inside the slice (6 + 2 wherever the slice holds them -- what feeds one engine best, profiles/r05_driver_shares.md --,
    6 + 1 on 8 cores)."""
    from conftest import pkg
    E = pkg("eval_rcnn")
    cores = list(range(ncores))
    per = ncores // 8
    seen = []
    for r in range(8):
        b = E.host_budget(world=8, local_rank=r, cores=cores)
        assert b["cores"] == list(range(per * r, per * r + per))
        assert b["loaders"] >= 1 and b["writers"] >= 1 and b["loaders"] + b["writers"] + 1 <= per
        seen += b["cores"]
    assert seen == cores
    want = {256: (6, 2), 128: (6, 2), 64: (6, 1)}[ncores]
    assert (b["loaders"], b["writers"]) == want


def test_slice_topology_of_a_two_socket_smt_host():
    """round 6: a rank's share of the REAL machine is a run of physical cores of the NUMA node its GPU hangs off plus their SMT siblings
    (EPYC numbering: first hardware threads 0 .. 127 across both sockets, siblings 128 .. 255 -- a contiguous id range is neither), the
    shares of 8 ranks are disjoint and cover the host, and a single rank's pin set is 32 neighbouring physical cores of node 0."""
    from conftest import pkg
    E = pkg("eval_rcnn")
    topo = [[(c, c + 128) for c in range(0, 64)], [(c, c + 128) for c in range(64, 128)]]
    seen = []
    for r in range(8):
        mine = E.slice_topology(topo, 8, r)
        node = 0 if r < 4 else 1
        lo = 64 * node + 16 * (r % 4)
        assert mine == list(range(lo, lo + 16)) + list(range(lo + 128, lo + 144))
        seen += mine
    assert sorted(seen) == list(range(256))
    one = E.slice_topology(topo, 1, 0)
    assert one[:E.PIN_CORES] == list(range(32)) and len(one) == 128          # node 0: physical cores first
    two = [E.slice_topology(topo, 2, r) for r in range(2)]
    assert two[0][:64] == list(range(64)) and two[1][:64] == list(range(64, 128))


def test_all_gather_is_identity_without_process_group():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import pkg
    E = pkg("eval_rcnn")
    t, c = torch.zeros((2, 4, 9)), torch.tensor([1, 0], dtype=torch.int32)
    t2, c2 = E.all_gather_detections(t, c, torch.device("cpu"))
    assert t2 is t and c2 is c


def _ap_worker(rank, world, port, q):
    try:
        import importlib
        import torch.distributed as dist
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from oracle import ext_cpu
        import test_kitti_eval as TK
        E = importlib.import_module("3d_adapt_auto_driving_amd.eval_rcnn")
        # every rank holds the detections of ITS scenes (here: the generator's own car boxes), rank r = scenes r, r+W, ...
        E_, src, table, counts = TK.synthetic_perfect_table(16)
        mine = E.shard_scene_ids(16, rank, world)
        t, c = E.all_gather_detections(table[mine].contiguous(), counts[mine].contiguous(), "cpu")
        out = None
        if rank == 0:                       # the AP tail runs where the gathered table lands
            with ext_cpu.patch_package():
                text, ret = E.evaluate_detections(t, c, src)
            out = (tuple(t.shape), sorted(int(v) for v in t[:, 0, 8].tolist()), float(ret["Car_3d_moderate"]),
                   float(ret["Car_bev_moderate"]), text.splitlines()[0])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        q.put((rank, "ERR " + traceback.format_exc()))


def test_sharded_detections_gathered_then_ap_on_rank0():
    """Config 4 end to end on CPU: scenes sharded over 2 ranks, one all_gather of the padded tables, rank 0 turns the
    gathered table into KITTI annotations and computes the AP (rotated IoU through the oracle stand-in): every scene
    arrives exactly once and perfect detections score 100."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ap_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(60)
    assert not isinstance(res[0], str) or not res[0].startswith("ERR"), res[0]
    assert not isinstance(res[1], str) or not str(res[1]).startswith("ERR"), res[1]
    shape, ids, ap3d, apbev, head = res[0]
    assert shape[0] == 16 and ids == list(range(16))
    assert abs(ap3d - 100.0) < 1e-9 and abs(apbev - 100.0) < 1e-9
    assert head.startswith("Car AP@0.70, 0.70, 0.70")


def test_host_budget_splits_the_node_between_ranks():
    """8 ranks on a 128-core node: disjoint contiguous 16-core slices (GPU r on the cores of its own socket half), and a loader /
    writer count that fits the slice instead of 16 + 6 processes per rank (176 host processes with no placement)."""
    from conftest import pkg
    E = pkg("eval_rcnn")
    cores = list(range(128))
    seen = set()
    for r in range(8):
        b = E.host_budget(world=8, local_rank=r, cores=cores)
        assert b["cores"] == list(range(16 * r, 16 * r + 16))
        assert not (seen & set(b["cores"]))
        seen |= set(b["cores"])
        assert b["loaders"] + b["writers"] + 1 <= 16 and b["loaders"] == 6 and b["writers"] == 2
    one = E.host_budget(world=1, local_rank=0, cores=cores)
    assert one["cores"] == cores and one["loaders"] == 6 and one["writers"] == 2         # round 5: 6 + 2 feed one engine best (16 + 6 until then)
    tiny = E.host_budget(world=8, local_rank=5, cores=list(range(4)))                    # more ranks than cores: still valid
    assert tiny["loaders"] >= 1 and tiny["writers"] >= 1 and tiny["cores"]


def test_host_budget_is_idempotent_after_pinning(monkeypatch):
    """eval_scenes calls host_budget() + pin_to_budget() on every invocation; the second call must slice the node's
    ORIGINAL affinity again (same cores), not the slice the first call pinned the process to (128 -> 16 -> 2 -> 1)."""
    import os
    from conftest import pkg
    E = pkg("eval_rcnn")
    node = list(range(64))
    state = {"aff": set(node)}
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(state["aff"]))
    monkeypatch.setattr(os, "sched_setaffinity", lambda pid, cores: state.__setitem__("aff", set(cores)))
    monkeypatch.setattr(os, "cpu_count", lambda: 64)
    monkeypatch.setattr(pkg("host"), "_NODE_AFFINITY", None)
    first = E.host_budget(world=4, local_rank=2)
    assert first["cores"] == list(range(32, 48))
    assert E.pin_to_budget(first) and state["aff"] == set(range(32, 48))
    for _ in range(3):
        again = E.host_budget(world=4, local_rank=2)
        assert again["cores"] == first["cores"] and again["loaders"] == first["loaders"]
        E.pin_to_budget(again)
    # a rank its launcher already confined to a quarter of the node keeps the quarter whole
    monkeypatch.setattr(pkg("host"), "_NODE_AFFINITY", None)
    state["aff"] = set(range(16, 32))
    kept = E.host_budget(world=4, local_rank=3)
    assert kept["cores"] == list(range(16, 32))
