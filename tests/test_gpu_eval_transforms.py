"""The fused best-match launch (prcnn_bev_best_match) and the device alignment pass (prcnn_eval_align) of csrc/eval_match.hip, and
evaluate(device="cuda") on top of them, against (a) the pair matrices of prcnn_rotate_iou_eval_segmented with numpy's max / argmax
and (b) fixture g17, the reference's own evaluate/evaluate.py (tests/golden/make_golden_eval_transforms.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg, ROOT, PKG_NAME
import eval_transforms_tree as T

pytestmark = pytest.mark.gpu


def fused(boxes_list, query_list, criterion, columns=True):
    """prcnn_bev_best_match on per-segment box lists -> row_val, row_idx, col_val, col_idx (host; columns None when not asked)."""
    import torch
    L = pkg("_lib")
    n = np.array([len(b) for b in boxes_list]); k = np.array([len(q) for q in query_list])
    box_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32); q_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 5) for x in xs], 0))
    dev = torch.device("cuda", 0)
    b, q = torch.from_numpy(cat(boxes_list)).to(dev), torch.from_numpy(cat(query_list)).to(dev)
    bo, qo = torch.from_numpy(box_off).to(dev), torch.from_numpy(q_off).to(dev)
    rv = torch.full((int(n.sum()),), -7.0, device=dev); ri = torch.full((int(n.sum()),), -7, dtype=torch.int32, device=dev)
    cv = torch.full((int(k.sum()),), -7.0, device=dev) if columns else None
    ci = torch.full((int(k.sum()),), -7, dtype=torch.int32, device=dev) if columns else None
    L.call("prcnn_bev_best_match", len(boxes_list), int(n.sum()), int(k.sum()), bo.data_ptr(), qo.data_ptr(), b.data_ptr(), q.data_ptr(),
           int(criterion), rv.data_ptr(), ri.data_ptr(), L.ptr(cv), L.ptr(ci), L.current_stream(b))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(rv), host(ri), host(cv), host(ci)


def dense(boxes_list, query_list, criterion):
    """The same from the pair matrices: np.max / np.argmax per block, value 0 and index -1 where a side is empty."""
    KE = pkg("kitti_eval")
    blocks, _ = KE.rotate_iou_segmented(boxes_list, query_list, criterion)
    rv, ri, cv, ci = [], [], [], []
    for o in blocks:
        assert o.dtype == np.float32
        if o.shape[0] and o.shape[1]:
            rv.append(o.max(1)); ri.append(o.argmax(1)); cv.append(o.max(0)); ci.append(o.argmax(0))
        else:
            rv.append(np.zeros(o.shape[0], np.float32)); ri.append(np.full(o.shape[0], -1))
            cv.append(np.zeros(o.shape[1], np.float32)); ci.append(np.full(o.shape[1], -1))
    c = np.concatenate
    return c(rv), c(ri).astype(np.int32), c(cv), c(ci).astype(np.int32)


def bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def sweep_segments(seed):
    """Segment sizes 0..400 on both sides, one-sided empty segments, planted exact duplicates on both sides."""
    rng = np.random.default_rng(seed)
    sizes = [(0, 0), (0, 7), (9, 0), (1, 1), (1, 400), (400, 1), (400, 400), (16, 16), (17, 15), (63, 65), (64, 64), (130, 33), (10, 6),
             (300, 60), (5, 129), (0, 1), (1, 0), (33, 257)]
    sizes += [(int(rng.integers(0, 401)), int(rng.integers(0, 401))) for _ in range(6)]

    def boxes(m, spread):
        return np.stack([rng.uniform(-spread, spread, m), rng.uniform(-spread, spread, m), rng.uniform(1.2, 2.4, m),
                         rng.uniform(2.5, 5.5, m), rng.uniform(-np.pi, np.pi, m)], 1).astype(np.float32)
    bl, ql = [], []
    for n, k in sizes:
        spread = 3.0 + 0.06 * max(n, k)
        b, q = boxes(n, spread), boxes(k, spread)
        if n >= 2 and k >= 2:
            m = min(n, k) // 2
            q[:m] = b[:m] + np.float32([0.2, -0.1, 0, 0, 0.05])      # real matches
            q[k - 1] = q[0]                                           # an exact duplicate query: a tie along the row ...
            b[n - 1] = b[0]                                           # ... and an exact duplicate box: a tie along the column
            if k >= 4:
                q[k // 2] = q[1]
        bl.append(b); ql.append(q)
    return bl, ql


@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
def test_fused_best_match_equals_the_pair_matrix_sweep(criterion):
    bl, ql = sweep_segments(100 + criterion)
    want = dense(bl, ql, criterion)
    got = fused(bl, ql, criterion)
    assert bit_equal(got[0], want[0]) and bit_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    ties = sum(int(((o == o.max(1, keepdims=True)).sum(1) > 1)[o.max(1) > 0].sum())
               for o in pkg("kitti_eval").rotate_iou_segmented(bl, ql, criterion)[0] if o.size)
    assert ties >= 10                                                   # the lowest-index rule was exercised
    rows_only = fused(bl, ql, criterion, columns=False)                # the column outputs are NULL-able
    assert rows_only[2] is None and bit_equal(rows_only[0], want[0]) and np.array_equal(rows_only[1], want[1])


def test_fused_best_match_on_the_fixture_and_empty_inputs():
    KE = pkg("kitti_eval")
    z = T.fixture()
    gt, dt = T.annos(z)
    bl, ql = [KE._bev_boxes(a) for a in dt], [KE._bev_boxes(a) for a in gt]
    got, want = fused(bl, ql, -1), dense(bl, ql, -1)
    assert bit_equal(got[0], want[0]) and bit_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    dm, gm = KE.best_match(dt, gt, device="cuda")
    for matches, key in ((dm, "bm_dt"), (gm, "bm_gt")):                 # ... and equal to the reference's recorded pairs
        assert np.array_equal(np.concatenate([v for v, _ in matches]), z[key + "_val"])
        assert np.array_equal(np.concatenate([i for _, i in matches]), z[key + "_idx"])
    e = np.zeros((0, 5), np.float32)
    assert [x.shape for x in fused([e], [e], -1)] == [(0,)] * 4
    assert KE.best_match([], [], device="cuda") == ([], [])
    with pytest.raises(pkg("_lib").PrcnnError):
        fused([e], [e], 3)


def random_annos(seed, n_img=40):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for i in range(n_img):
        k = 0 if i == 3 else int(rng.integers(1, 40))
        loc = np.stack([rng.uniform(-30, 30, k), rng.uniform(1.2, 2.0, k), rng.uniform(2, 75, k)], 1)
        dim = np.stack([rng.normal(3.9, 0.5, k), rng.normal(1.6, 0.15, k), rng.normal(1.7, 0.15, k)], 1)
        ry = rng.uniform(-np.pi, np.pi, k)
        gts.append({"name": np.array(["Car"] * k), "location": loc, "dimensions": dim, "rotation_y": ry})
        n = 0 if i == 5 else k + int(rng.integers(0, 6))
        pick = rng.integers(0, max(k, 1), n)
        dl = (loc[pick] if k else rng.uniform(-30, 30, (n, 3))) + rng.normal(0, 0.5, (n, 3)) * rng.choice([0.1, 1, 6], (n, 1))
        dd = (dim[pick] if k else np.tile([3.9, 1.6, 1.7], (n, 1))) * rng.uniform(0.7, 1.4, (n, 3))
        dts.append({"name": np.array(["Car"] * n), "location": dl, "dimensions": dd,
                    "rotation_y": (ry[pick] if k else np.zeros(n)) + rng.normal(0, 0.2, n), "alpha": rng.uniform(-7, 7, n)})
    return gts, dts


def check_alignment(make):
    KE = pkg("kitti_eval")
    for mode in (0, 1):
        gt_a, dt_a = make()
        gt_b, dt_b = make()
        br_dev = np.concatenate(KE._align(dt_a, gt_a, mode, "cuda", 0))
        br_np = np.concatenate(KE._align(dt_b, gt_b, mode, "cpu", 0))     # numpy statements over the pair matrices
        assert np.array_equal(br_dev, br_np)                              # who was aligned, and by which branch
        cat = lambda annos, key: np.concatenate([a[key] for a in annos], 0)
        assert np.array_equal(cat(dt_a, "dimensions"), cat(dt_b, "dimensions"))           # copies: bit for bit
        # location: the only inexact operations are f64 sin / cos / atan2 (an ulp between device and host); shifts of a few metres on
        # coordinates below 100 m (ulp 1.4e-14): 1e-12 m is about 70 ulp of slack
        assert np.abs(cat(dt_a, "location") - cat(dt_b, "location")).max() <= 1e-12
        touched = br_np >= 0
        assert touched.sum() >= 20 and (~touched).sum() >= 5
        if mode == 1:
            for bit, both in ((1, 2), (4, 8)):
                taken = touched & (br_np & bit > 0)
                assert (taken & (br_np & both > 0)).any() and (taken & (br_np & both == 0)).any()
        else:
            assert set(br_np.tolist()) == {-1, 0} and np.array_equal(cat(dt_a, "location"), cat(dt_b, "location"))
    return br_np


def test_device_alignment_equals_numpy_on_the_fixture():
    z = T.fixture()
    br = check_alignment(lambda: T.annos(z))
    assert np.array_equal(br, z["front_branch"])


def test_device_alignment_equals_numpy_on_a_sweep():
    check_alignment(lambda: random_annos(7))


@pytest.mark.parametrize("name", T.CONFIG_NAMES)
def test_configuration_matches_reference_gpu(name, tmp_path):
    z = T.fixture()
    T.check_configuration(z, name, dict(T.configs(z))[name], tmp_path, "cuda")


def test_command_line_module_on_the_gpu(tmp_path):
    z = T.fixture()
    t = T.write_tree(z, tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", PKG_NAME + ".kitti_eval", "--result_path", t["result"], "--dataset_path", t["dataset"],
                        "--align_size", "--toground", "--direct_save", "--device", "cuda"], capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout == str(z["text_size_ground_save"]) + "\n"
    assert T.written(t)[0] == [str(n) for n in z["files_size_ground_save_names"]]
