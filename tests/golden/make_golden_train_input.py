"""Generates tests/golden/g20_train_input_ref.npz: RPN training batches as the REFERENCE's own KittiRCNNDataset(mode='TRAIN') and
collate_batch make them for tests/train_tree.py's fake tree, with the database its own tools/generate_gt_database.py makes of that tree.

RUN IN THE BUILD CONTAINER ONLY (imports the reference through ref_harness, read-only; needs scipy and oracle/_ref):
    python tests/golden/make_golden_train_input.py
kitti_utils.get_iou3d runs over shapely_shim.py in place of shapely.  An accept decision must not rest on the
stand-in's last bits, so every tested pair must be apart (still disjoint with the new box grown by 0.05 m on every side, or no height
overlap within 0.05 m) or overlap with IoU >= 1e-3; the generator fails otherwise.

Two recordings from np.random.seed(SEED) each, one process, dataset[i] in order, batches [0, 1, 2] and [3, 4, 5, 6]:
  a   GT_AUG_HARD_RATIO 0.6 (easy and hard list), GT_AUG_RAND_NUM
  b   GT_AUG_HARD_RATIO 0, GT_EXTRA_NUM 15 without GT_AUG_RAND_NUM: 16 candidates reach the test in every augmented scene (the cap)
both with GT_AUG_ENABLED, GT_AUG_APPLY_PROB 0.75, AUG_DATA, npoints 1024, npoints_faraway 128.
  <r>_<batch>_<key>       every array entry of the collated batch;  <r>_<batch>_aug_method  repr of the list
  <r>_state_keys / <r>_state_pos / ...    np.random.get_state() after the recording
  <r>_decisions           (sample id, accepted, max IoU, database entry) per overlap test;  <r>_pos the entries' obj.pos after the
                          recording (the drift);  <r>_hard_ratio;  <r>_rand_num;  seed;  numpy;  cases (json)
"""
import json
import logging
import pickle
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402
import shapely_shim  # noqa: E402

SEED = int(sys.argv[1]) if len(sys.argv) > 1 else 2020         # the committed fixture: the default
GROUPS = ([0, 1, 2], [3, 4, 5, 6])


def grown(corners, d):
    """the bottom quad of a corner array with every side moved out by d (a rectangle: along its two edge directions)"""
    q = corners[0:4][:, [0, 2]].astype(np.float64)
    c = q.mean(0)
    out = []
    for p in q:
        v = p - c
        e1, e2 = q[1] - q[0], q[3] - q[0]
        u1, u2 = e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
        out.append(p + d * (np.sign(v @ u1) * u1 + np.sign(v @ u2) * u2))
    return np.array(out)


def record(name, hard_ratio, rand_num, tree, db_file, out, cases):
    from lib.config import cfg
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    import lib.utils.kitti_utils as K
    import train_tree
    cfg.GT_AUG_ENABLED, cfg.GT_AUG_RAND_NUM, cfg.GT_AUG_APPLY_PROB, cfg.GT_AUG_HARD_RATIO = True, rand_num, 0.75, hard_ratio
    cfg.GT_EXTRA_NUM = 15
    cfg.AUG_DATA, cfg.RPN.ENABLED, cfg.RCNN.ENABLED, cfg.RPN.FIXED, cfg.RPN.USE_INTENSITY = True, True, False, False, True
    ds = KittiRCNNDataset(root_dir=tree, npoints=train_tree.NPOINTS, split=train_tree.SPLIT, mode="TRAIN", classes="Car",
                          logger=logging.getLogger("g20"), gt_database_dir=db_file, npoints_faraway=train_tree.NPOINTS_FARAWAY)
    assert [int(i) for i in ds.sample_id_list] == list(train_tree.SAMPLE_IDS)
    decisions, cur = [], {"id": None, "n_orig": None, "entries": []}
    calls_before = cases["aug_calls"]
    entries = (ds.gt_database[0] + ds.gt_database[1]) if hard_ratio > 0 else ds.gt_database
    centres = np.array([[e["gt_box3d"][0], e["gt_box3d"][2]] for e in entries], dtype=np.float64)
    orig = {tuple(np.round(c, 4)): k for k, c in enumerate(np.array([[e["gt_box3d"][0], e["gt_box3d"][2]] for e in
                                                                   pickle.load(open(db_file, "rb"))], dtype=np.float64))}
    assert len(orig) == len(entries), "two database entries share a centre"
    iou_fn, aug_fn, rand_fn = K.get_iou3d, ds.apply_gt_aug_to_one_scene, np.random.rand

    def w_iou(a, b):
        r = iou_fn(a, b)
        if cur["n_orig"] is None:
            cur["n_orig"] = b.shape[0]
        n0 = cur["n_orig"]
        for j in range(b.shape[0]):
            if r[0, j] >= 1e-3:
                continue
            assert r[0, j] == 0, "a pair inside the band 0 < IoU < 1e-3: change the tree or the seed (%r)" % r[0, j]
            big = shapely_shim.Polygon(grown(a[0], 0.05))
            apart = big.intersection(shapely_shim.Polygon(b[j, 0:4][:, [0, 2]])).area == 0.0
            ha = (-a[0, 0:4, 1].mean(), -a[0, 4:8, 1].mean())
            hb = (-b[j, 0:4, 1].mean(), -b[j, 4:8, 1].mean())
            apart = apart or min(ha[1], hb[1]) - max(ha[0], hb[0]) <= -0.05
            assert apart, "a disjoint pair closer than 0.05 m: change the tree or the seed"
        ok = bool(r.max() < 1e-8)
        c = a[0, 0:4][:, [0, 2]].astype(np.float64).mean(0)
        entry = orig[tuple(np.round(centres[np.argmin(((centres - c) ** 2).sum(1))], 4))]
        if entry in cur["entries"]:
            cases["entry_drawn_twice"] += 1
        cur["entries"].append(entry)
        if not ok:
            cases["rejected_original" if r[0, :n0].max() >= 1e-8 else "rejected_accepted_only"] += 1
            plain = shapely_shim.Polygon(grown(a[0], -0.25))
            if all(plain.intersection(shapely_shim.Polygon(grown(b[j], -0.25))).area == 0.0 for j in range(b.shape[0])):
                cases["rejected_enlargement_only"] += 1
        else:
            cases["accepted"] += 1
        cases["tests"] += 1
        decisions.append((cur["id"], int(ok), float(r.max()), entry))
        return r

    def w_aug(sample_id, *a):
        cur["id"], cur["n_orig"], cur["entries"] = int(sample_id), None, []
        before = len(decisions)
        cases["aug_calls"] += 1
        if a[2].shape[0] > 64:
            cases["more_than_64_boxes"] += 1
        r = aug_fn(sample_id, *a)
        cases["max_tests_per_scene"] = max(cases["max_tests_per_scene"], len(decisions) - before)
        n_new = r[1].shape[0]
        cur["n_final"] = n_new
        return r

    flag_fn = ds.get_valid_flag

    def w_flag(*a):
        f = flag_fn(*a)
        cur["n_final"] = int(f.sum())                        # the cloud the sampler sees unless GT-aug changes it (w_aug)
        return f

    K.get_iou3d, ds.apply_gt_aug_to_one_scene, ds.get_valid_flag = w_iou, w_aug, w_flag
    if hard_ratio > 0:
        cases["easy_entries"], cases["hard_entries"] = len(ds.gt_database[0]), len(ds.gt_database[1])
    try:
        np.random.seed(SEED)
        for gi, group in enumerate(GROUPS):
            samples = []
            for i in group:
                samples.append(ds[i])
                n_new = cur["n_final"]
                cases["cloud_over_npoints"] += n_new > train_tree.NPOINTS
                cases["cloud_under_npoints"] += train_tree.NPOINTS // 2 <= n_new < train_tree.NPOINTS
                cases["cloud_under_half"] += n_new < train_tree.NPOINTS // 2
            for smp in samples:
                m = smp.get("aug_method", [])
                kinds = [x if isinstance(x, str) else x[0] for x in m]
                for kind in ("rotation", "scaling", "flip"):
                    cases[kind + ("_taken" if kind in kinds else "_not_taken")] += 1
            batch = ds.collate_batch(samples)
            for key, v in batch.items():
                out["%s_%d_%s" % (name, gi, key)] = np.array(repr(v)) if key == "aug_method" else np.asarray(v)
        st = np.random.get_state()
    finally:
        K.get_iou3d = iou_fn
    cases["skipped_by_apply_prob"] += len(sum(GROUPS, [])) - (cases["aug_calls"] - calls_before)
    out[name + "_state_key"], out[name + "_state_rest"] = np.asarray(st[1]), np.array([st[2], st[3], st[4]], dtype=np.float64)
    out[name + "_decisions"] = np.array(decisions, dtype=np.float64).reshape(-1, 4)
    pos = np.zeros((len(entries), 3), dtype=np.float32)
    for e in entries:
        pos[orig[(round(float(e["gt_box3d"][0]), 4), round(float(e["gt_box3d"][2]), 4))]] = e["obj"].pos
    out[name + "_pos"] = pos
    out[name + "_rand_num"] = np.int64(rand_num)
    if not rand_num:
        per = {}
        for d in decisions:
            per[d[0]] = per.get(d[0], 0) + 1
        assert max(per.values()) == 16, "no scene reaches the cap of 16 candidates"
        cases["cap_16_reached"] += 1
    out[name + "_hard_ratio"] = np.float64(hard_ratio)
    print(name, cases)


def main():
    H.install()
    shapely_shim.install()
    from oracle import oracle
    ref = oracle.load_reference_roipool()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    sys.modules["roipool3d_cuda"] = ref
    sys.path.append(os.path.join(H.REF, "tools"))
    import train_tree
    out = {"seed": np.int64(SEED), "numpy": np.array(np.__version__)}
    keys = ("accepted", "rejected_original", "rejected_accepted_only", "tests", "aug_calls", "more_than_64_boxes", "max_tests_per_scene",
            "cloud_over_npoints", "cloud_under_npoints", "cloud_under_half", "skipped_by_apply_prob", "easy_entries", "hard_entries",
            "rejected_enlargement_only", "entry_drawn_twice", "cap_16_reached",
            "rotation_taken", "rotation_not_taken", "scaling_taken", "scaling_not_taken", "flip_taken", "flip_not_taken")
    cases = {k: 0 for k in keys}
    with tempfile.TemporaryDirectory() as tree:
        train_tree.write_train_tree(tree)
        db_dir = os.path.join(tree, "db")
        argv, cwd = sys.argv, os.getcwd()
        tool = os.path.join(H.REF, "tools", "generate_gt_database.py")
        sys.argv = [tool, "--root", tree, "--save_dir", db_dir, "--class_name", "Car"]
        try:
            os.chdir(tree)
            runpy.run_path(tool, run_name="__main__")
        finally:
            sys.argv = argv
            os.chdir(cwd)
        (db_file,) = os.listdir(db_dir)
        for name, ratio, rand_num in (("a", 0.6, True), ("b", 0.0, False)):
            record(name, ratio, rand_num, tree, os.path.join(db_dir, db_file), out, cases)
    for key in keys:
        assert cases[key] > 0, "the run contains no case of: %s" % key
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "g20_train_input_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
