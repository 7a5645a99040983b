"""Random object scaling on the device (csrc/object_scale.hip through object_scale.scale_objects and RpnTrainInput obj_scale) against
the numpy definition, bit for bit: the operator at the shapes where the kernel can go wrong (one point, a ragged last workgroup, box
counts around the LDS chunk of 16, counts below G, an empty scene), and the training input stage per key with both random streams."""
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import object_scale_scenes as scenes  # noqa: E402
import test_gpu_train_input as TGI  # noqa: E402
from test_gpu_train_input import tree_db  # noqa: E402,F401  (the module's fixture: train_tree's tree and its GT database)

PKG = "3d_adapt_auto_driving_amd"
pytestmark = pytest.mark.gpu


def mod(name):
    return importlib.import_module(PKG + "." + name)


# ---------------------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("B, N, G, C, counts", [
    (1, 1, 1, 3, None),
    (1, 257, 1, 4, None),                        # a second workgroup of one point
    (3, 300, 17, 3, [17, 9, 16]),                # one box past the first chunk; counts below G and on the chunk
    (2, 1024, 33, 4, [33, 32]),                  # one box past the second chunk
    (2, 64, 4, 3, [0, 4]),                       # a scene without boxes
])
def test_operator_equals_the_definition(B, N, G, C, counts):
    """(g)"""
    OS = mod("object_scale")
    pts, gt, counts, factors = scenes.operator_case(100 + N + G, B, N, G, counts)
    if N > 1:
        pts[0, 0] = 0.0                                                        # the exact origin: inside every zero row, were it visited
    inten = np.random.default_rng(3).random((B, N, 1), dtype=np.float32)
    extra = np.concatenate((pts, inten), axis=2) if C == 4 else pts.copy()
    for fac in ([factors] if G > 1 else [factors, np.full((B, 1), 1.125)]):         # with one box the 1.0 leaves nothing to move: both
        check_operator(OS, pts, gt, counts, fac, extra, inten if C == 4 else None)


def check_operator(OS, pts, gt, counts, factors, extra, inten):
    import torch
    (B, N), G = pts.shape[:2], gt.shape[1]
    want_p, want_g, want_h = OS.scale_objects(pts, gt, counts, factors, device="cpu")
    t_pts, t_extra = torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(extra.copy()).cuda()
    got_p, got_g, got_h = OS.scale_objects(t_pts, gt, counts, factors, device="cuda", extra=t_extra)
    assert got_p.data_ptr() == t_pts.data_ptr() and torch.is_tensor(got_h) and got_h.is_cuda          # in place, on the device
    gp, gh, ge = got_p.cpu().numpy(), got_h.cpu().numpy(), t_extra.cpu().numpy()
    assert gh.dtype == np.uint32 and gh.shape == (B, G) and gh.tobytes() == want_h.tobytes()
    assert gp.tobytes() == want_p.tobytes()
    assert isinstance(got_g, np.ndarray) and got_g.tobytes() == want_g.tobytes()
    assert np.ascontiguousarray(ge[:, :, :3]).tobytes() == want_p.tobytes()
    if inten is not None:
        assert ge[:, :, 3:].tobytes() == inten.tobytes()
    # what the case is there for: owned points that move and owned points whose factor is 1.0, nothing counted past a count
    live = np.arange(G)[None, :] < counts[:, None]
    assert (want_h[~live] == 0).all() and int(want_h.sum()) <= B * N
    if N >= 64:
        assert int(want_h.sum()) > 0 and (want_h[live & (factors == 1.0)] > 0).any() == bool((factors == 1.0).any())
        assert (want_p != pts).any() == bool((factors[live] != 1.0).any())
    if G >= 2 and N >= 257:
        assert (want_h[:, 0] > 0).all() and (want_h[:, 1] > 0).all()                                  # the overlapping pair: both own points


def test_operator_without_extra_and_on_a_host_array():
    """a numpy ``pts`` is uploaded (and left alone); no ``extra``"""
    OS = mod("object_scale")
    pts, gt, counts, factors = scenes.operator_case(9, 2, 500, 5)
    keep = pts.copy()
    want_p, _, want_h = OS.scale_objects(pts, gt, counts, factors, device="cpu")
    got_p, _, got_h = OS.scale_objects(pts, gt, counts, factors, device="cuda")
    assert pts.tobytes() == keep.tobytes()
    assert got_p.cpu().numpy().tobytes() == want_p.tobytes() and got_h.cpu().numpy().tobytes() == want_h.tobytes()


# -------------------------------------------------------------------------------------------------------------------- the stage
def same_streams(a, b):
    TGI.same_state(a, b)
    sa, sb = a.scale_generator_state(), b.scale_generator_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert a.last_scaled == b.last_scaled and len(a.last_scaled) > 0


def source(tree_db, cfg, device, seed, npoints, faraway, with_replace, **kw):  # noqa: F811
    T = mod("train_input")
    return T.RpnTrainInput(tree_db[0], cfg, tree_db[1], split=TGI.train_tree.SPLIT, npoints=npoints, npoints_faraway=faraway,
                           with_replace=with_replace, seed=seed, device=device, **kw)


@pytest.mark.parametrize("hard_ratio, intensity, npoints, faraway, with_replace, groups, seed", [
    (0.6, True, 1024, 128, False, ([0, 1, 2, 3, 4], [5, 6]), 2020),          # B = 5
    (0.0, False, 256, 32, False, ([6], [3], [1]), 7),                        # B = 1, npoints 256, the aug-scene id, no intensity
    (0.6, True, 1024, 128, True, ([2, 0, 5],), 11),                          # with_replace; scene 2 has more than 64 label boxes
])
def test_stage_device_equals_cpu(tree_db, hard_ratio, intensity, npoints, faraway, with_replace, groups, seed):  # noqa: F811
    """(h) the rows of test_gpu_train_input.test_device_equals_cpu with obj_scale=(0.8, 1.2)"""
    cfg = TGI.make_cfg(hard_ratio, intensity)
    dev = source(tree_db, cfg, "cuda", seed, npoints, faraway, with_replace, obj_scale=(0.8, 1.2))
    cpu = source(tree_db, cfg, "cpu", seed, npoints, faraway, with_replace, obj_scale=(0.8, 1.2))
    scaled = 0
    for group in groups:
        got = dev.batch(group)
        TGI.same(got, cpu.batch(group))
        same_streams(dev, cpu)
        assert got["pts_rect"].is_cuda and got["pts_input"].is_cuda
        scaled += sum(rec[3] for rec in dev.last_scaled if rec[2] != 1.0)
    assert scaled > 0                                                         # points were moved


def test_stage_option_off_is_byte_equal_on_the_device(tree_db):  # noqa: F811
    """(i) obj_scale=(1.0, 1.0) on the device against the device run without the option"""
    cfg = TGI.make_cfg()
    plain = source(tree_db, cfg, "cuda", 2020, 1024, 128, False)
    ones = source(tree_db, cfg, "cuda", 2020, 1024, 128, False, obj_scale=(1.0, 1.0))
    for group in ([0, 1, 2, 3, 4], [5, 6]):
        TGI.same(ones.batch(group), plain.batch(group))
        TGI.same_state(ones, plain)
        assert plain.last_scaled == [] and ones.last_scaled and all(rec[2] == 1.0 for rec in ones.last_scaled)
