"""CPU: the f64 definition of the training layer (tests/train_layer_ref.py) against torch.autograd in f64 on torch's own
Conv1d + BatchNorm1d(train) + ReLU, to 1e-10 of each tensor's largest magnitude (both sides are f64 evaluations of one formula; sums
of a few thousand terms leave about 1e-13); the lattice generator's promises; and the switch's pass-through on what it does not cover."""
import numpy as np
import pytest
import torch

import train_layer_ref as R
from conftest import pkg

FORMS = [(True, True), (True, False), (False, True), (False, False)]        # (bn, relu)


def close(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err, mag = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= 1e-10 * max(mag, 1e-300), "%s: err %.3e at magnitude %.3e" % (what, err, mag)


def random_case(b, cin, cout, p, bn, relu, seed):
    rng = np.random.default_rng(seed)
    case = dict(x=rng.standard_normal((b, cin, p)), w=rng.standard_normal((cout, cin)), dy=rng.standard_normal((b, cout, p)),
                eps=1e-5, momentum=0.1, bn=bn, relu=relu, gamma=None, beta=None, bias=None)
    if bn:
        case.update(gamma=rng.standard_normal(cout), beta=rng.standard_normal(cout), running_mean=rng.standard_normal(cout),
                    running_var=rng.uniform(0.5, 2.0, cout))
    else:
        case["bias"] = rng.standard_normal(cout)
    return case


@pytest.mark.parametrize("bn,relu", FORMS)
@pytest.mark.parametrize("shape", [(1, 3, 16, 2), (3, 19, 13, 63), (2, 33, 20, 257)])
def test_definition_against_torch_autograd_in_f64(shape, bn, relu):
    case = random_case(*shape, bn, relu, seed=sum(shape) + 2 * bn + relu)
    want, got = R.torch_block(case, torch.float64), R.reference(case)
    assert set(got) == set(want)
    for key in sorted(want):
        close(key, got[key], want[key])


def test_definition_on_a_lattice_case_with_a_zero_weight_row():
    case = R.lattice_case(2, 19, 16, 63, zero_row=5)
    want, got = R.torch_block(case, torch.float64), R.reference(case)
    assert got["rstd"][5] == 1.0 / np.sqrt(1e-5) and got["mean"][5] == 0.0
    for key in sorted(want):
        assert np.isfinite(got[key]).all()
        close(key, got[key], want[key])


@pytest.mark.parametrize("bn,relu", FORMS)
@pytest.mark.parametrize("shape", [(1, 3, 16, 2), (3, 19, 130, 63), (2, 131, 196, 257), (3, 6, 16, 2051), (2, 96, 32, 1027)])
def test_lattice_cases_are_exact_in_f32_and_keep_the_margin(shape, bn, relu):
    case = R.lattice_case(*shape, bn=bn, relu=relu)
    for key in ("x", "w"):
        assert case[key].dtype == np.float32 and np.array_equal(case[key] * 8, np.round(case[key] * 8)) and np.abs(case[key]).max() <= 2
    fw = R.forward(case["x"], case["w"], case["gamma"], case["beta"], case["bias"], case["eps"], relu)
    assert np.array_equal(fw["z"], fw["z"].astype(np.float32).astype(np.float64))
    # an f32 chain in another order gives the same z: every partial sum is exact
    z32 = np.zeros(fw["z"].shape, np.float32)
    for ci in reversed(range(shape[1])):
        z32 += case["w"][None, :, ci, None] * case["x"][:, None, ci, :]
    assert np.array_equal(z32.astype(np.float64), fw["z"])
    assert case["margin"] >= R.MARGIN and float(np.abs(fw["pre"]).min()) == case["margin"]
    if relu and shape[0] * shape[3] > 2:
        on = (fw["pre"] > 0).mean()
        assert 0.2 < on < 0.8, "the threshold sits near the median: both sides of the mask are exercised"


def test_switch_is_off_by_default_and_passes_through_what_it_does_not_cover():
    pt = pkg("pointnet2.pytorch_utils")
    assert pt.FUSED_TRAIN_LAYERS is False
    torch.manual_seed(0)
    mlp = pt.SharedMLP([6, 16, 32], bn=True).train()
    x = torch.randn(2, 6, 37, 5)
    state = {k: v.clone() for k, v in mlp.state_dict().items()}
    want = mlp(x)
    after = {k: v.clone() for k, v in mlp.state_dict().items()}
    mlp.load_state_dict(state)
    with pt.fused_train_layers():
        assert pt.FUSED_TRAIN_LAYERS is True
        tl = pkg("pointnet2.train_layer")
        assert not tl.covers(mlp[0], x), "a CPU tensor is not covered"
        got = mlp(x)                                   # CPU tensors: torch's modules, exactly as before
        with pt.fused_train_layers(False):
            assert pt.FUSED_TRAIN_LAYERS is False
        assert pt.FUSED_TRAIN_LAYERS is True
    assert pt.FUSED_TRAIN_LAYERS is False
    assert torch.equal(got, want)
    for k, v in mlp.state_dict().items():
        assert v.dtype == after[k].dtype and torch.equal(v, after[k]), k


def test_train_rcnn_accepts_and_logs_fused_layers(tmp_path):
    """The parser, and main() up to the input stage -- which finds no tree under an empty root -- by which time the arguments are logged."""
    T = pkg("train_rcnn")
    assert T.build_parser().parse_args(["--train_mode", "rpn", "--root", "r"]).fused_layers is False
    assert T.build_parser().parse_args(["--train_mode", "rpn", "--root", "r", "--fused_layers"]).fused_layers is True
    logs = {}
    for flag in ([], ["--fused_layers"]):
        out = tmp_path / ("out%d" % len(flag))
        with pytest.raises(Exception):
            T.main(["--train_mode", "rpn", "--root", str(tmp_path / "empty"), "--output_dir", str(out), "--device", "cpu"] + flag)
        logs[len(flag)] = (out / "log_train.txt").read_text()
    assert "fused_layers" not in logs[0] and "Start logging" in logs[0]
    assert logs[1].count("fused_layers True") == 1
    assert pkg("pointnet2.pytorch_utils").FUSED_TRAIN_LAYERS is False


def test_header_constant_and_prototypes():
    L = pkg("_lib")
    assert L.PRCNN_TRAIN_CHUNK == L.ENUMS["PRCNN_TRAIN_CHUNK"] and L.PRCNN_TRAIN_CHUNK % 256 == 0
    for name in ("prcnn_train_layer_workspace", "prcnn_train_layer_forward", "prcnn_train_layer_backward"):
        assert name in L.SIGNATURES
