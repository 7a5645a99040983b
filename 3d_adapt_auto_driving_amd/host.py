"""The share of the host a rank's processes may use: CPU topology from sysfs, the rank's cores, loader / writer counts, pinning."""
import os

import torch


_NODE_AFFINITY = None          # the affinity this process STARTED with (captured once: eval_scenes may run several times per process)


def _node_affinity():
    global _NODE_AFFINITY
    if _NODE_AFFINITY is None:
        try:
            _NODE_AFFINITY = sorted(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            _NODE_AFFINITY = list(range(os.cpu_count() or 1))
    return _NODE_AFFINITY


def _cpu_topology(allowed):
    """-> [[(physical cpu, sibling, ...), ...] per NUMA node], restricted to ``allowed``, from sysfs; None when it cannot be read.
    (EPYC hosts number the first hardware threads 0 .. P-1 across the sockets and the SMT siblings P .. 2P-1: a CONTIGUOUS range of CPU
    ids is not a set of neighbouring cores -- on the 2 x 64-core MI355X boxes ids 64-127 are the OTHER socket, 128-191 the siblings of 0-63.)"""
    import glob

    def parse(text):
        out = []
        for part in text.strip().split(","):
            if part:
                lo, _, hi = part.partition("-")
                out += range(int(lo), int(hi or lo) + 1)
        return out
    try:
        allowed = set(allowed)
        nodes = []
        for path in sorted(glob.glob("/sys/devices/system/node/node[0-9]*/cpulist"), key=lambda q: int(q.split("node")[-1].split("/")[0])):
            with open(path) as f:
                cpus = [c for c in parse(f.read()) if c in allowed]
            groups, seen = [], set()
            for c in cpus:
                if c in seen:
                    continue
                with open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c) as f:
                    sib = [x for x in parse(f.read()) if x in allowed]
                seen.update(sib)
                groups.append(tuple(sorted(sib)))
            if groups:
                nodes.append(groups)
        if {c for n in nodes for t in n for c in t} != allowed:     # sysfs does not describe the CPUs we were given: no topology
            return None
        return nodes or None
    except (OSError, ValueError):
        return None


def slice_topology(topo, world, k):
    """rank k of ``world`` local ranks on a host of ``topo`` (= _cpu_topology): the ranks are dealt to the NUMA nodes in order (GPUs
    0 .. W/2-1 hang off node 0, the rest off node 1 on the 2-socket MI355X hosts), a node's PHYSICAL cores are cut into equal runs, and
    a rank gets its run's first hardware threads followed by their SMT siblings -> list of CPU ids, physical cores first."""
    rpn = -(-world // len(topo))                                       # ranks per node
    node = min(k // rpn, len(topo) - 1)
    groups = topo[node]
    on_node = max(1, min(rpn, world - node * rpn))
    gper = max(1, len(groups) // on_node)
    g = groups[(k % rpn) * gper:(k % rpn) * gper + gper] or groups
    return [t[0] for t in g] + [c for t in g for c in t[1:]]


PIN_CORES = 32      # CPUs a rank's processes are confined to (profiles/r06_driver_sweep.md: the whole driver on 32 cores of the GPU's socket
#                     runs 5800-6200 scenes/s on the KITTI tree, on 64 cores 5000-5400, unconfined on 256 CPUs 4500-5600)


def host_budget(world=None, local_rank=None, cores=None):
    """The share of the host one rank may use when W ranks of a node each drive a GPU with loader and writer processes
    (at 16 loaders + 6 writers per rank, 8 ranks are 176 processes on 128-256 cores with no placement).
    -> dict: cores (the CPU ids of this rank: a contiguous slice of the node's CPUs -- on the MI355X hosts GPUs 0-3 hang off
    socket 0 and 4-7 off socket 1, and Linux numbers a socket's cores contiguously, so the slice stays on the GPU's NUMA node),
    loaders, writers.  PRCNN_LOADER_WORKERS / PRCNN_WRITER_PROCS override the counts, PRCNN_NO_AFFINITY=1 the pinning."""
    world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) if world is None else int(world)
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if local_rank is None else int(local_rank)
    world = max(1, world)
    topo_ok = cores is None
    if cores is None:
        # always sliced from the affinity the process started with, never from a slice an earlier call pinned it to (ADVICE r3:
        # 128 cores became 16, then 2, then 1 over repeated eval_scenes calls); a rank its launcher already confined to a 1/W share
        # of the node (or less) keeps that share whole
        cores = _node_affinity()
        if world > 1 and len(cores) * world <= (os.cpu_count() or 0):
            world_slices = 1
        else:
            world_slices = world
    else:
        world_slices = world
    per = max(1, len(cores) // world_slices)
    k = local_rank % world_slices
    mine = cores[k * per:k * per + per] or cores
    pin = None
    if topo_ok:
        # the real machine: a rank's share = a run of PHYSICAL cores of one NUMA node (GPUs 0 .. W/2-1 hang off node 0, the rest off
        # node 1) plus their SMT siblings, physical cores first; the processes are pinned to the first PIN_CORES of it
        topo = _cpu_topology(cores)
        if topo:
            mine = slice_topology(topo, world_slices, k)
            pin = mine[:PIN_CORES]
    # one core for the thread that feeds the GPU, a quarter of the rest for the writers (text formatting), the rest for the loaders --
    # at most 6 + 2 (round 5, profiles/r05_driver_shares.md: the whole driver runs 5260-5400 scenes/s with 6 loaders + 2 writers,
    # 4550-5110 with 8 + 2, 3800-3900 with 8-10 + 3 and 3200-3600 with the 16 + 6 of rounds 2-4 on the same 256-core box: beyond what
    # the engine consumes, more producer processes only add wake-ups and pinned-memory traffic around the one thread that feeds the GPU)
    spare = max(1, len(mine) - 1)
    writers = max(1, min(2, spare // 4))
    loaders = max(1, min(6, spare - writers))
    if pin is None:                                     # no topology (or an explicit core list): a single rank takes the head of its cores
        pin = mine[:PIN_CORES] if world_slices == 1 else mine
    return {"cores": mine, "pin": pin,
            "loaders": int(os.environ.get("PRCNN_LOADER_WORKERS", loaders)),
            "writers": int(os.environ.get("PRCNN_WRITER_PROCS", writers)), "world": world, "local_rank": local_rank}


def pin_to_budget(budget):
    """Restrict this process (and the loader / writer processes it starts: affinity is inherited) to the rank's cores -- since round 6
    also a single rank, to budget["pin"]: PIN_CORES neighbouring cores next to its GPU.  eval_scenes restores the previous affinity
    when it returns.  PRCNN_NO_AFFINITY=1: leave the affinity alone."""
    if os.environ.get("PRCNN_NO_AFFINITY") == "1":
        return False
    try:
        os.sched_setaffinity(0, budget.get("pin") or budget["cores"])
        return True
    except (AttributeError, OSError):
        return False


def _limit_worker_threads(_worker_id=None):
    """Start-up hook of every loader / writer process: ONE thread for the numeric libraries.  A loader's numpy work is a few small
    products per scene (Calibration.lidar_to_rect: (n, 4) x (4, 3)); left alone, each of them fans out over the BLAS / OpenMP pool of
    the whole host (256 threads on the MI355X boxes) -- processes x cores runnable threads around the one thread that feeds the GPU.
    PRCNN_LOADER_THREADS (default 1; 0: leave the libraries alone)."""
    n = int(os.environ.get("PRCNN_LOADER_THREADS", "1"))
    if n <= 0:
        return
    try:
        torch.set_num_threads(n)
    except RuntimeError:
        pass
    try:
        import threadpoolctl
        global _THREAD_LIMIT
        _THREAD_LIMIT = threadpoolctl.threadpool_limits(limits=n)      # kept alive: the limit lasts as long as the object
    except Exception:                                                   # noqa: BLE001 -- no threadpoolctl: the environment variables below
        pass


_THREAD_LIMIT = None
