"""The engine's structure, pinned from outside: which weight tensors a freshly built FastPointRCNN holds (names, order, shapes --
before any forward has run), that reload_weights() brings every one of them to a fresh engine's bits without a forward in between,
and (-m gpu) which extension entries one default.yaml forward reaches, in order.  The golden lists are this project's own output,
recorded before the engine's scale / level tuples became records (tests/golden/engine_weight_tensors.json,
tests/golden/engine_calls_default.json); the one stated difference is that the joint per-point weights of RPN SA2's two narrow
scales (sa._pcat[0], sa._pcat[1]) exist from construction on instead of from the first GPU forward on."""
import json
import os

import pytest
import torch

from conftest import pkg
from test_eval_sweep import _randomised
from test_host_logic import tiny_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _default_model(device="cpu", seed=0):
    cfg = pkg("config").default_eval_cfg()
    return pkg("eval_rcnn").build_model(cfg, device, seed=seed), cfg


def held(eng):
    return [[n, list(t.shape)] for n, t in eng.weight_tensors()]


@pytest.mark.parametrize("which", ["default", "tiny", "tiny_intensity"])
def test_a_fresh_engine_holds_the_golden_weight_tensors(which):
    F = pkg("net.fast_infer")
    if which == "default":
        model, cfg = _default_model()
    else:
        model, cfg, _ = tiny_model(intensity=which == "tiny_intensity")
    got = held(F.FastPointRCNN(model, cfg))                    # no forward
    want = _golden("engine_weight_tensors.json")[which]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert got == want
    if which == "default":
        # the joint narrow-pair weights close the list: (K, 128) and (128,), K the padded width of SA1's output
        assert got[-2:] == [["sa._pcat[0]", [128, 128]], ["sa._pcat[1]", [128]]]
    else:
        assert not any(n.startswith("sa._pcat") for n, _ in got)


def test_reload_rewrites_the_joint_narrow_pair_weights_without_a_forward():
    F = pkg("net.fast_infer")
    model, cfg = _default_model()
    eng = F.FastPointRCNN(model, cfg)
    before = [(n, t.data_ptr(), t.clone()) for n, t in eng.weight_tensors()]
    model.load_state_dict(_randomised(model, 21))
    eng.reload_weights()                                        # no forward before, none after
    fresh = F.FastPointRCNN(model, cfg)
    mine, new = eng.weight_tensors(), fresh.weight_tensors()
    assert [n for n, _ in mine] == [n for n, _ in new]
    pcat = [(n, t, t2) for (n, t), (_, t2) in zip(mine, new) if n.startswith("sa._pcat")]
    assert [n for n, _, _ in pcat] == ["sa._pcat[0]", "sa._pcat[1]"]
    for n, t, t2 in pcat:
        assert torch.equal(t, t2), n
    for (n, t), (_, t2), (_, ptr, was) in zip(mine, new, before):
        assert torch.equal(t, t2) and t.data_ptr() == ptr, n   # every form: a fresh engine's bits at the old address
    assert all(not torch.equal(t, was) for (n, t), (_, _, was) in zip(mine, before) if n.startswith("sa._pcat"))


# ---------------------------------------------------------------------------------------------------------------- calls of one forward
class Recorder:
    """pass-through proxy around one extension module: appends the name of every entry that is called to `log` (predicates
    `*_supported` and classes such as PrefixExpected are host-side helpers, not entries: handed through as they are)"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or isinstance(fn, type) or name.endswith("_supported"):
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def recorded_forward_calls(device="cuda:0"):
    """the ordered entry names one forward() of the default.yaml engine (seed-0 model, default switches) reaches on B = 2 scenes
    of cfg.RPN.NUM_POINTS points"""
    F, S = pkg("net.fast_infer"), pkg("synth")
    pu, ru, iu = pkg("pointnet2.pointnet2_utils"), pkg("roipool3d_utils"), pkg("iou3d_utils")
    model, cfg = _default_model(device)
    eng = F.FastPointRCNN(model, cfg)
    pts = torch.from_numpy(S.scenes(2, cfg.RPN.NUM_POINTS, seed0=31)).to(device)
    log = []
    saved = (pu.pointnet2, ru.roipool3d_cuda, iu.iou3d_cuda)
    pu.pointnet2, ru.roipool3d_cuda, iu.iou3d_cuda = (Recorder(m, log) for m in saved)
    try:
        out = eng.forward(pts)
        torch.cuda.synchronize()
    finally:
        pu.pointnet2, ru.roipool3d_cuda, iu.iou3d_cuda = saved
    assert torch.isfinite(out["rcnn_cls"]).all() and torch.isfinite(out["rcnn_reg"]).all()
    return log


@pytest.mark.gpu
def test_one_default_forward_reaches_the_golden_entries_in_order():
    got = recorded_forward_calls()
    want = _golden("engine_calls_default.json")
    assert len(want) > 20
    assert got == want
