"""The order-fixed backward without a GPU: the numpy definitions of tests/scatter_ref.py against a literal per-slot loop, the new
entries' argument checks, the header constant, and train_rcnn's --ordered_backward (parsed, logged; silent without it)."""
import numpy as np
import pytest

import scatter_ref as R
from conftest import pkg


def case():
    rng = np.random.default_rng(11)
    b, n, slots, c = 3, 257, 592, 7
    idx = rng.integers(0, n, (b, slots)).astype(np.int32)
    idx[1] = 5                                                   # every slot on one point: one list of 592, 256 empty lists
    idx[2, rng.choice(slots, 40, replace=False)] = -1            # out of range on both sides: no list
    idx[2, rng.choice(slots, 40, replace=False)] = n
    terms = rng.standard_normal((b, c, slots)).astype(np.float32)
    return idx, terms, n


@pytest.mark.parametrize("chunk", [4, 256])
def test_numpy_definitions_equal_the_literal_loop(chunk):
    idx, terms, n = case()
    offsets, entries = R.plan(idx, n)
    want_off, want_lists, want_sums = R.literal(idx, terms, n, chunk)
    assert np.array_equal(offsets, want_off)
    for i in range(len(idx)):
        assert entries[i][:offsets[i][n]].tolist() == [s for lst in want_lists[i] for s in lst]
    assert offsets[1][6] - offsets[1][5] == 592 and 592 - 80 <= offsets[2][n] == int(((idx[2] >= 0) & (idx[2] < n)).sum()) < 592
    got = R.ordered_sum(offsets, entries, terms, n, chunk)
    assert np.array_equal(R.bits(got), R.bits(want_sums))
    if chunk == 4:                                               # the chunk rule changes bits: it is exercised, not decoration
        assert not np.array_equal(R.bits(got), R.bits(R.ordered_sum(offsets, entries, terms, n, 1 << 20)))


def test_plan_of_nothing():
    for shape, n in (((0, 6), 4), ((2, 0), 4), ((2, 3, 0), 1)):
        offsets, entries = R.plan(np.zeros(shape, np.int32), n)
        assert offsets.shape == (shape[0], n + 1) and not offsets.any() and entries.shape == (shape[0], int(np.prod(shape[1:])))
    assert R.ordered_sum(*R.plan(np.zeros((2, 0), np.int32), 4), np.zeros((2, 3, 0), np.float32), 4, 256).shape == (2, 3, 4)


def test_interp_terms_are_the_f32_products_by_slot():
    rng = np.random.default_rng(3)
    g, w = rng.standard_normal((2, 3, 5)).astype(np.float32), rng.random((2, 5, 3)).astype(np.float32)
    t = R.interp_terms(g, w)
    assert t.shape == (2, 3, 15) and t.dtype == np.float32
    for s in range(15):
        assert np.array_equal(t[:, :, s], g[:, :, s // 3] * w[:, s // 3, s % 3][:, None])


def test_ordered_entries_reject_bad_arguments_without_gpu():
    L = pkg("_lib")
    with pytest.raises(L.PrcnnError, match="null pointer"):
        L.call("prcnn_scatter_plan", 1, 8, 8, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="bad sizes"):
        L.call("prcnn_scatter_plan", 1, -1, 8, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="bad sizes"):
        L.call("prcnn_scatter_plan_workspace", 1, 8, -1)
    assert L.call("prcnn_scatter_plan_workspace", 3, 257, 592) >= 1 and L.call("prcnn_scatter_plan_workspace", 0, 0, 0) >= 1
    with pytest.raises(L.PrcnnError, match="null pointer"):
        L.call("prcnn_group_points_grad_ordered", 1, 2, 8, 8, 2, 0, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="bad sizes"):
        L.call("prcnn_group_points_grad_ordered", 1, -2, 8, 8, 2, 0, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="bad sizes"):                     # channels c0 .. c0+c-1 must lie inside c_total
        L.call("prcnn_group_points_grad_ordered", 1, 4, 8, 8, 6, 3, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="null pointer"):
        L.call("prcnn_three_interpolate_grad_ordered", 1, 2, 8, 4, None, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="bad sizes"):
        L.call("prcnn_three_interpolate_grad_ordered", 1, 2, 8, -4, None, None, None, None, None, None)


def test_chunk_constant_comes_from_the_header():
    L = pkg("_lib")
    assert "PRCNN_SCATTER_CHUNK" in L.ENUMS and L.PRCNN_SCATTER_CHUNK == L.ENUMS["PRCNN_SCATTER_CHUNK"] >= 1
    for name in ("prcnn_scatter_plan_workspace", "prcnn_scatter_plan", "prcnn_group_points_grad_ordered",
                 "prcnn_three_interpolate_grad_ordered"):
        assert name in L.SIGNATURES


def test_switch_is_off_by_default_and_scoped():
    pu = pkg("pointnet2.pointnet2_utils")
    assert pu.ORDERED_BACKWARD is False
    with pu.ordered_backward():
        assert pu.ORDERED_BACKWARD is True
        with pu.ordered_backward(False):
            assert pu.ORDERED_BACKWARD is False
        assert pu.ORDERED_BACKWARD is True
    assert pu.ORDERED_BACKWARD is False
    with pytest.raises(KeyError):
        with pu.ordered_backward():
            raise KeyError("x")
    assert pu.ORDERED_BACKWARD is False


def test_train_rcnn_accepts_and_logs_ordered_backward(tmp_path):
    """No CPU stand-in runs the whole loop, so: the parser, and main() up to the input stage -- which finds no tree under an empty
    root -- by which time the arguments are logged."""
    T = pkg("train_rcnn")
    assert T.build_parser().parse_args(["--train_mode", "rpn", "--root", "r"]).ordered_backward is False
    assert T.build_parser().parse_args(["--train_mode", "rpn", "--root", "r", "--ordered_backward"]).ordered_backward is True
    logs = {}
    for flag in ([], ["--ordered_backward"]):
        out = tmp_path / ("out%d" % len(flag))
        with pytest.raises(Exception):
            T.main(["--train_mode", "rpn", "--root", str(tmp_path / "empty"), "--output_dir", str(out), "--device", "cpu"] + flag)
        logs[len(flag)] = (out / "log_train.txt").read_text()
    assert "ordered_backward" not in logs[0] and "Start logging" in logs[0]
    assert logs[1].count("ordered_backward True") == 1
