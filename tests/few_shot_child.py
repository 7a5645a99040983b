"""Child process of tests/test_few_shot.py: one rank of a world of two over gloo, on the CPU.

  few_shot_child.py RANK PORT ROOT SHUFFLE OUT.json

train_rcnn.resolve_sample_ids for ``--subsample 3 --shuffle_subsample SHUFFLE`` under the group.  On every rank but 0
scene_batch.sample_id_list -- the call that writes a missing train_car1_<S>.txt from an unseeded shuffle -- raises: only rank 0 may
reach it.  Writes {"rank", "ids", "path"} to OUT.json and prints one JSON line {"ok": true}."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

PKG = "3d_adapt_auto_driving_amd"


def main(rank, port, root, shuffle, out_file):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    T = importlib.import_module(PKG + ".train_rcnn")
    D = importlib.import_module(PKG + ".dist_train")
    SB = importlib.import_module(PKG + ".scene_batch")
    a = T.build_parser().parse_args(["--train_mode", "rpn", "--root", root, "--device", "cpu", "--subsample", "3", "--shuffle_subsample", shuffle])
    cfg = T.make_cfg(a)
    group = D.ReplicaGroup.from_env("cpu", "gloo")
    assert group.active and group.rank == rank
    if rank != 0:
        def never(*args, **kw):
            raise AssertionError("rank %d resolved the sample list itself" % rank)
        SB.sample_id_list = never
    try:
        ids, path = T.resolve_sample_ids(a, cfg, group)
    finally:
        group.close()
    with open(out_file, "w") as f:
        json.dump({"rank": rank, "ids": ids, "path": path}, f)
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5])
