"""-m gpu end-to-end parity: the model on the GPU (HIP operators through the C ABI, PyTorch-ROCm
convolutions) against the same model on the CPU with the oracle operator backend, and against the
fixture recorded from the REFERENCE model (tests/golden/g8_e2e_tiny_ref.npz).

Tolerance (BASELINE.json north_star): indices bit-exact, box regressions within 1e-4.  The
convolutions run in different libraries on the two sides (MIOpen/rocBLAS f32 vs MKL f32), so head
outputs agree to ~1e-5 and an index decision (arg-max bin, sort order, NMS) could flip on a
near-tie; the fixtures are built so that they do not (make_golden.py spreads the head weights),
and the full-size test matches boxes one-to-one instead of assuming identical ordering."""
import importlib

import numpy as np
import pytest
import torch

from conftest import pkg
from test_host_logic import tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_tiny_model_gpu_matches_reference_fixture():
    model, cfg, g = tiny_model(DEV)
    det = pkg("eval_rcnn").infer_batch(model, cfg, torch.from_numpy(g["pts"]).to(DEV))
    np.testing.assert_allclose(det["rois"].cpu().numpy(), g["rois"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(det["rcnn_reg"].cpu().numpy(), g["rcnn_reg"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(det["rcnn_cls"].cpu().numpy(), g["rcnn_cls"], rtol=0, atol=1e-4)
    assert np.array_equal(det["num"].cpu().numpy(), g["final_num"])                    # NMS keep counts
    np.testing.assert_allclose(det["boxes"].cpu().numpy(), g["final_boxes"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(det["scores"].cpu().numpy(), g["final_scores"], rtol=0, atol=1e-4)


def test_tiny_model_with_intensity_gpu_matches_reference_fixture(tmp_path):
    """cfg.RPN.USE_INTENSITY = True, pts_input (B, N, 4): the nn.Module graph over the HIP operators against the fixture recorded from
    the REFERENCE model in that configuration (g8i), and the whole driver on such a configuration (make_runner -> ModuleRunner)"""
    E = pkg("eval_rcnn")
    model, cfg, g = tiny_model(DEV, intensity=True)
    det = E.infer_batch(model, cfg, torch.from_numpy(g["pts"]).to(DEV))
    np.testing.assert_allclose(det["rois"].cpu().numpy(), g["rois"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(det["rcnn_reg"].cpu().numpy(), g["rcnn_reg"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(det["rcnn_cls"].cpu().numpy(), g["rcnn_cls"], rtol=0, atol=1e-4)
    assert np.array_equal(det["num"].cpu().numpy(), g["final_num"])
    np.testing.assert_allclose(det["boxes"].cpu().numpy(), g["final_boxes"], rtol=0, atol=1e-4)
    # round 4: the point-major engine covers the configuration (general kernels; EngineRunner): same fixture, same tolerance
    runner = E.make_runner(model, cfg, DEV)
    assert isinstance(runner, E.EngineRunner)
    de = E.infer_batch(model, cfg, torch.from_numpy(g["pts"]).to(DEV), engine=runner.engine)
    for key, ref in (("rois", "rois"), ("rcnn_cls", "rcnn_cls"), ("rcnn_reg", "rcnn_reg"), ("boxes", "final_boxes"), ("scores", "final_scores")):
        np.testing.assert_allclose(de[key].cpu().numpy(), g[ref], rtol=0, atol=1e-4)
    assert np.array_equal(de["num"].cpu().numpy(), g["final_num"])
    src = pkg("kitti_io").SyntheticSource(cfg, 5)
    table, counts = E.eval_scenes(model, cfg, DEV, src, src.ids, batch_size=2, output_dir=str(tmp_path), workers=0)
    assert table.shape[0] == 5 and len(list(tmp_path.glob("*.txt"))) == 5
    one = E.infer_batch(model, cfg, torch.from_numpy(np.stack([src.load(i)[0] for i in (0, 1)])).to(DEV))
    n0 = int(one["num"][0])
    assert int(counts[0]) == n0 and np.allclose(table[0, :n0, :7], one["boxes"][0, :n0].cpu().numpy(), atol=1e-5)


def test_fast_engine_gpu_matches_reference_fixture_and_pipelining_is_transparent():
    """Point-major engine on the GPU vs the reference fixture; and the two-stream pipelined runner
    returns exactly what the same engine returns when called serially."""
    E, F = pkg("eval_rcnn"), pkg("net.fast_infer")
    model, cfg, g = tiny_model(DEV)
    pts = torch.from_numpy(g["pts"]).to(DEV)
    eng = F.FastPointRCNN(model, cfg)
    det = E.infer_batch(model, cfg, pts, engine=eng)
    for key, ref in (("rois", "rois"), ("rcnn_cls", "rcnn_cls"), ("rcnn_reg", "rcnn_reg"),
                     ("boxes", "final_boxes"), ("scores", "final_scores")):
        np.testing.assert_allclose(det[key].cpu().numpy(), g[ref], rtol=0, atol=1e-4)
    assert np.array_equal(det["num"].cpu().numpy(), g["final_num"])
    runner = E.PipelinedRunner(model, cfg, DEV)
    other = torch.from_numpy(pkg("synth").scenes(2, 2048, seed0=123)).to(DEV)
    seq = [pts, other, pts, other, pts]
    outs = [runner.step(seq[i], seq[i + 1] if i + 1 < len(seq) else None) for i in range(len(seq))]
    torch.cuda.synchronize()
    for i in (0, 2, 4):
        assert torch.equal(outs[i]["boxes"], det["boxes"]) and torch.equal(outs[i]["num"], det["num"])
    ref_other = E.infer_batch(model, cfg, other, engine=eng)
    assert torch.equal(outs[1]["boxes"], ref_other["boxes"]) and torch.equal(outs[3]["scores"], ref_other["scores"])
    # three-stream form (tails beside the GEMM stream, RCNN of batch i-1 after RPN of batch i): same results, one
    # batch later
    runner3 = E.PipelinedRunner(model, cfg, DEV)
    lag = [runner3.submit(seq[i], seq[i + 1] if i + 1 < len(seq) else None) for i in range(len(seq))]
    lag = lag[1:] + [runner3.flush()]
    assert lag[-1] is not None and runner3.flush() is None
    for i, d in enumerate(lag):
        d["ready"].synchronize()
        want = det if i % 2 == 0 else ref_other
        for key in ("boxes", "scores", "num", "rois", "rcnn_cls"):
            assert torch.equal(d[key], want[key]), (i, key)


def test_xyz_level_kernel_equals_gemm_chain_in_engine():
    """Full-size RPN backbone with the first SA level through csrc/sa_xyz_mlp.hip vs through the grouped GEMM
    chain: the (B, N, 128) point features agree to f32 rounding."""
    C, E, F = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer")
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, DEV, seed=0)
    eng = F.FastPointRCNN(model, cfg)
    pts = torch.from_numpy(pkg("synth").scenes(2, cfg.RPN.NUM_POINTS, seed0=77)).to(DEV)
    geo = eng.geometry(pts)
    a = eng._backbone(pts, geo)
    F.USE_XYZ_MLP = False
    try:
        b = eng._backbone(pts, geo)
    finally:
        F.USE_XYZ_MLP = True
    assert torch.isfinite(a).all() and float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
    assert float(a.abs().max()) > 0


def test_roipool_canonical_kernel_equals_torch_sequence():
    """RCNN input assembly in one kernel (enlarge + pool + canonical transform + aligned rows) vs the reference-order
    sequence pool -> subtract centre -> rotate -> pad: the pooled coordinates agree to 1 ulp-level rounding (the torch
    path rotates through a batched matmul), features / mask / depth rows are identical, an empty box holds the image
    of the origin in both, and the RCNN heads agree to 1e-5."""
    C, E, F = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer")
    RU = pkg("roipool3d_utils")
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, DEV, seed=0)
    eng = F.FastPointRCNN(model, cfg)
    B, N = 2, cfg.RPN.NUM_POINTS
    pts = torch.from_numpy(pkg("synth").scenes(B, N, seed0=91)).to(DEV)
    st = eng.rpn_stage(pts)
    rois, _ = eng.propose(st)
    rois = rois.clone()
    rois[0, 3, 0:3] = torch.tensor([5.0, -40.0, 30.0], device=DEV)             # 40 m above the scene: certainly empty
    # kernel-level comparison of the pooled tensor
    feats, mask, depth = st["rpn_features"], st["seg_result"], (st["pts_depth"] / 70.0 - 0.5).contiguous()
    M, S, Cf = rois.shape[1], cfg.RCNN.NUM_POINTS, feats.shape[2]
    pooled = torch.full((B, M, S, 8 + Cf), float("nan"), device=DEV)
    empty = torch.full((B, M), -1, dtype=torch.int32, device=DEV)
    RU.roipool3d_cuda.forward_canonical(pts, rois.contiguous(), feats, mask.contiguous(), depth, cfg.RCNN.POOL_EXTRA_WIDTH, pooled, empty)
    ref_in = torch.cat([mask.unsqueeze(2), depth.unsqueeze(2), feats], dim=2)
    ref, ref_empty = RU.roipool3d_gpu(pts, ref_in, rois, cfg.RCNN.POOL_EXTRA_WIDTH, sampled_pt_num=S)
    assert torch.equal(empty, ref_empty) and int(empty[0, 3]) == 1 and int(empty.sum()) >= 1
    assert torch.equal(pooled[..., 3:5], ref[..., 3:5]) and torch.equal(pooled[..., 8:], ref[..., 5:])
    assert bool((pooled[..., 5:8] == 0).all())
    ref_xyz = ref[..., 0:3] - rois[:, :, 0:3].unsqueeze(2)
    ref_xyz = pkg("kitti_utils").rotate_pc_along_y_torch(ref_xyz.reshape(B * M, S, 3), rois.reshape(-1, 7)[:, 6]).view(B, M, S, 3)
    dxyz = (pooled[..., 0:3] - ref_xyz).abs()
    print("canonical xyz: max |diff| %.3g, differing elements %d of %d" % (float(dxyz.max()), int((dxyz > 0).sum()), dxyz.numel()))
    assert float(dxyz.max()) < 2e-5                                            # |coordinates| <= ~50 m: a few ulp at most
    # through the RCNN; and the MFMA entrance chain (csrc/rcnn_entrance.hip) vs the library GEMMs + concat
    a = eng.rcnn_stage(st, rois)
    F.USE_RCNN_POINT_MLP = False
    try:
        c = eng.rcnn_stage(st, rois)
        F.USE_ROIPOOL_CANONICAL = False
        b = eng.rcnn_stage(st, rois)
    finally:
        F.USE_ROIPOOL_CANONICAL = True
        F.USE_RCNN_POINT_MLP = True
    for k in ("rcnn_cls", "rcnn_reg"):
        scale = max(1.0, float(c[k].abs().max()))
        assert float((a[k] - c[k]).abs().max()) <= 5e-5 * scale, ("point_mlp", k, float((a[k] - c[k]).abs().max()), scale)
    for k in ("rcnn_cls", "rcnn_reg"):
        scale = max(1.0, float(b[k].abs().max()))
        assert float((a[k] - b[k]).abs().max()) <= 5e-5 * scale, (k, float((a[k] - b[k]).abs().max()), scale)


def test_backbone_indices_bit_exact_full_size(oracle):
    """FPS / ball-query indices of all four RPN SA levels on a full 16384-point scene: the xyz chain
    involves no convolution, so GPU and oracle must agree exactly at every level."""
    pu = pkg("pointnet2.pointnet2_utils")
    xyz = pkg("synth").scenes(2, 16384, seed0=40)
    cur_g, cur_c = torch.from_numpy(xyz).to(DEV), xyz
    for npoint, radii, ns in ((4096, (0.1, 0.5), (16, 32)), (1024, (0.5, 1.0), (16, 32)),
                              (256, (1.0, 2.0), (16, 32)), (64, (2.0, 4.0), (16, 32))):
        sel = pu.furthest_point_sample(cur_g, npoint)
        want = oracle.furthest_point_sample(cur_c, npoint)
        assert np.array_equal(sel.cpu().numpy(), want)
        new_g = pu.gather_operation(cur_g.transpose(1, 2).contiguous(), sel).transpose(1, 2).contiguous()
        new_c = np.take_along_axis(cur_c, want.astype(np.int64)[..., None].repeat(3, -1), 1)
        assert np.array_equal(new_g.cpu().numpy(), new_c)
        for r, s in zip(radii, ns):
            assert np.array_equal(pu.ball_query(r, s, cur_g, new_g).cpu().numpy(), oracle.ball_query(r, s, cur_c, new_c))
        cur_g, cur_c = new_g, new_c


def match_boxes(a, b):
    """greedy one-to-one matching of two (n,7) box sets by centre distance -> max abs diff of pairs"""
    if len(a) == 0 or len(b) == 0:
        return 0.0, 0
    d = np.linalg.norm(a[:, None, :3] - b[None, :, :3], axis=2)
    worst, used, matched = 0.0, set(), 0
    for i in np.argsort(d.min(1)):
        j = int(np.argmin(d[i]))
        if j in used or d[i, j] > 0.05:
            continue
        used.add(j); matched += 1
        worst = max(worst, float(np.abs(a[i] - b[j]).max()))
    return worst, matched


# (the full-size comparison of the nn.Module path with a CPU run of this build -- bars 1e-3 / 90 % of the RoIs -- is replaced by
#  tests/test_gpu_full_ref.py: module path AND engine against fixtures recorded from the REFERENCE model at default.yaml shapes,
#  1e-4 for every RoI and every final box)


def test_full_size_batch8_engine_gpu_vs_engine_on_cpu_oracle_every_box():
    """BASELINE configs[2] at its batch of 8, default.yaml shapes: the ENGINE on the GPU against the SAME engine code on CPU
    tensors with the oracle as operator backend (oracle/ext_cpu.py: scalar C restatements; the MLP kernels in their fixed
    fma-chain order).  Every operator this build owns is bit-exact against that backend (tests/test_gpu_shadow.py), so what
    is left between the two runs is (a) torch's elementwise glue (sigmoid, norm, reciprocal) and (b) f32 sin / cos of two
    libraries in the decoders -- no library GEMM is left on either side since the end of round 2 (every width is zero-padded to a
    multiple of 128 and runs on this build's layer kernels, whose order the oracle backend reproduces).  The bar of BASELINE.json's north
    star, for EVERY box: 100 % of the RoIs and 100 % of the final boxes matched one to one, within 1e-4; equal counts."""
    from oracle import ext_cpu
    C, E, F, S = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer"), pkg("synth")
    cfg = C.default_eval_cfg()
    model_c = E.build_model(cfg, "cpu", seed=3)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in model_c.named_parameters():
            if ("reg_layer" in name or "cls_layer" in name) and p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        model_c.rcnn_net.cls_layer[-1].conv.weight.mul_(0.05)
        model_c.rcnn_net.cls_layer[-1].conv.bias.fill_(0.5)
    model_g = E.build_model(cfg, DEV, seed=3)
    model_g.load_state_dict(model_c.state_dict())
    B = 8
    pts = torch.from_numpy(S.scenes(B, 16384, seed0=77))
    with ext_cpu.patch_package():
        dc = E.infer_batch(model_c, cfg, pts, engine=F.FastPointRCNN(model_c, cfg))
    dg = E.infer_batch(model_g, cfg, pts.to(DEV), engine=F.FastPointRCNN(model_g, cfg))
    assert torch.equal(dg["num"].cpu(), dc["num"]) and int(dc["num"].min()) >= 3
    assert float((dg["rois"].cpu() - dc["rois"]).abs().max()) <= 1e-4            # same RoIs in the same ORDER
    assert float((dg["rcnn_cls"].cpu() - dc["rcnn_cls"]).abs().max()) <= 1e-4
    worst_all = 0.0
    for b in range(B):
        n = int(dc["num"][b])
        worst, matched = match_boxes(dg["boxes"][b, :n].cpu().numpy(), dc["boxes"][b, :n].numpy())
        assert matched == n, (b, matched, n)
        worst_all = max(worst_all, worst)
        assert float((dg["boxes"][b, :n].cpu() - dc["boxes"][b, :n]).abs().max()) <= 1e-4   # ... and the same final order
        assert float((dg["scores"][b, :n].cpu() - dc["scores"][b, :n]).abs().max()) <= 1e-4
    assert worst_all <= 1e-4
    print("batch 8: %d final boxes, all matched, worst |d| = %.3g" % (int(dc["num"].sum()), worst_all))


def _seeded_full_model():
    """default.yaml PointRCNN with the seeded weights the reference-made fixture g12u was recorded with"""
    from test_host_logic import full_model
    model, cfg, g, pts = full_model(DEV, "u")
    return model, cfg, pts


def _run_both(model, cfg, pts, eng):
    """-> (engine run, module-path run) as (ret, det) pairs"""
    E = pkg("eval_rcnn")
    out = []
    with torch.no_grad():
        for use_engine in (True, False):
            ret = eng(pts) if use_engine else model({"pts_input": pts})
            if "seg_result" not in ret:
                ret["seg_result"] = (torch.sigmoid(ret["rpn_cls"][..., 0]) > cfg.RPN.SCORE_THRESH).float()
            out.append((ret, E.postprocess(cfg, ret, pts.shape[0])))
    torch.cuda.synchronize()
    return out


def test_full_size_engine_with_intensity_equals_module_path():
    """cfg.RPN.USE_INTENSITY at default.yaml shapes (the reference's CODE default, lib/config.py:40; (B, N, 4) input): the engine on
    its general kernels against the nn.Module graph, seeded weights, B = 2: every RoI, head output and final box within 1e-4."""
    import helpers
    C, E, F, S = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer"), pkg("synth")
    cfg = C.default_eval_cfg()
    C.merge_into({"RPN": {"USE_INTENSITY": True}}, cfg)
    model = E.build_model(cfg, "cpu")
    sd, _ = helpers.seeded_state_dict(model.state_dict(), 1204)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    pts = np.concatenate([S.scenes(2, cfg.RPN.NUM_POINTS, seed0=1204),
                          np.random.default_rng(5).random((2, cfg.RPN.NUM_POINTS, 1)).astype(np.float32) - np.float32(0.5)], axis=2)
    x = torch.from_numpy(pts).to(DEV)
    with torch.no_grad():
        # centre the segmentation threshold on the 70th percentile of the scores, as the fixtures do
        raw = model({"pts_input": x})["rpn_cls"]
        model.rpn.rpn_cls_layer[-1].conv.bias += float(-0.8473 - torch.quantile(raw.view(-1), 0.7))
    eng = F.FastPointRCNN(model, cfg)
    assert eng.in_feat == 1
    (ret_e, det_e), (ret_m, det_m) = _run_both(model, cfg, x, eng)
    rep = helpers.e2e_report(ret_e, det_e, helpers.e2e_record(ret_m, det_m))
    print("engine vs module path, USE_INTENSITY (B = 2):\n" + helpers.e2e_text(rep))
    assert all(r[2] == 0 for r in rep), helpers.e2e_text(rep)
    assert int(det_m["num"].min()) >= 3


def test_full_size_engine_is_complete_deterministic_and_equals_module_path():
    """default.yaml shapes, batch of 2: the point-major engine (fused MFMA / VALU kernels, ticket scheduling, all
    extension entry points) against the nn.Module graph on the same device and weights.
      * every torch.empty buffer is poisoned with NaN first: a tile or row that a kernel fails to write (a lost
        ticket, a short grid) surfaces as NaN in the heads;
      * two runs are bit-identical (no race, no stale memory);
      * EVERY RoI, head output and final box agrees with the module path within 1e-4, equal counts (round 3 held 1e-3 / 90 %
        here; both paths are also held to the reference-made fixture in tests/test_gpu_full_ref.py)."""
    import helpers
    E, F = pkg("eval_rcnn"), pkg("net.fast_infer")
    model, cfg, pts_np = _seeded_full_model()
    eng = F.FastPointRCNN(model, cfg)
    pts = torch.from_numpy(pts_np).to(DEV)
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    torch.empty = poisoned
    try:
        d1 = E.infer_batch(model, cfg, pts, engine=eng)
        d2 = E.infer_batch(model, cfg, pts, engine=eng)
    finally:
        torch.empty = real_empty
    for k in ("rois", "rcnn_cls", "rcnn_reg", "boxes", "scores"):
        assert torch.isfinite(d1[k]).all(), k
        assert torch.equal(d1[k], d2[k]), (k, float((d1[k] - d2[k]).abs().max()))
    (ret_e, det_e), (ret_m, det_m) = _run_both(model, cfg, pts, eng)
    rep = helpers.e2e_report(ret_e, det_e, helpers.e2e_record(ret_m, det_m))
    print("engine vs module path (B = 2):\n" + helpers.e2e_text(rep))
    assert all(r[2] == 0 for r in rep), helpers.e2e_text(rep)
    assert int(det_m["num"].min()) >= 10


@pytest.mark.parametrize("B", [1, 3])
def test_full_size_engine_other_batch_sizes(B):
    """The same engine-vs-module comparison at batch sizes 1 and 3 (tile counts that are not multiples of the workgroup
    quota, odd grids), three-stream runner included: 1e-4 on every RoI, head output and final box."""
    import helpers
    E, S = pkg("eval_rcnn"), pkg("synth")
    model, cfg, _ = _seeded_full_model()
    pts = torch.from_numpy(S.scenes(B, cfg.RPN.NUM_POINTS, seed0=300 + B)).to(DEV)
    runner = E.PipelinedRunner(model, cfg, DEV)
    assert runner.submit(pts, None) is None
    d1 = runner.flush()
    d1["ready"].synchronize()
    d2 = E.infer_batch(model, cfg, pts, engine=runner.engine)
    for k in ("rois", "rcnn_cls", "rcnn_reg", "boxes", "scores", "num"):
        assert torch.equal(d1[k], d2[k]), k
    (ret_e, det_e), (ret_m, det_m) = _run_both(model, cfg, pts, runner.engine)
    rep = helpers.e2e_report(ret_e, det_e, helpers.e2e_record(ret_m, det_m))
    print("engine vs module path (B = %d):\n" % B + helpers.e2e_text(rep))
    assert all(r[2] == 0 for r in rep), helpers.e2e_text(rep)
    assert int(det_m["num"].min()) >= 3


def test_pipelined_runner_full_size_many_steps_equals_serial():
    """Three-stream runner at default.yaml size over 14 steps of 4 different batches, geometry 3 batches ahead: every
    batch's detections are bit-identical to the serial engine's.  Guards the cross-stream hand-offs (events,
    record_stream of every tensor that changes streams -- including the packed row lists): a buffer recycled by the
    caching allocator while another stream still reads it shows up here as a differing or non-finite detection."""
    C, E, S = pkg("config"), pkg("eval_rcnn"), pkg("synth")
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, DEV, seed=3)
    runner = E.PipelinedRunner(model, cfg, DEV, depth=3)
    batches = [torch.from_numpy(S.scenes(8, cfg.RPN.NUM_POINTS, seed0=500 + 8 * k)).to(DEV) for k in range(4)]
    serial = [E.infer_batch(model, cfg, b, engine=runner.engine) for b in batches]
    torch.cuda.synchronize()
    steps = 14
    outs = []
    for i in range(steps):
        nxt = [batches[(i + d) % 4] for d in range(1, 4)]
        junk = [torch.empty((1 << 20,), device=DEV).fill_(float("nan")) for _ in range(3)]   # churn the allocator
        det = runner.submit(batches[i % 4], nxt)
        del junk
        if det is not None:
            outs.append(det)
    outs.append(runner.flush())
    torch.cuda.synchronize()
    assert len(outs) == steps
    for i, det in enumerate(outs):
        ref = serial[i % 4]
        for k in ("rois", "boxes", "scores", "num"):
            assert torch.equal(det[k], ref[k]), (i, k)


def test_roipool_culled_by_spatial_groups_equals_the_index_order_sweep():
    """forward_canonical with the scene's spatial groups (prcnn_point_groups: Morton-ordered points + per-group boxes) selects
    EXACTLY the points of the index-order sweep, in the same order: pooled rows, empty flags and distinct counts are bit-identical
    -- for ordinary RoIs, boxes far outside the scene, boxes on the scene's border, thin / tilted boxes, and boxes that hold more
    than 2048 points (those fall back to the sweep inside the kernel)."""
    C, S = pkg("config"), pkg("synth")
    RU = pkg("roipool3d_utils")
    cfg = C.default_eval_cfg()
    rng = np.random.default_rng(12)
    B, N, M, Cf, P = 3, cfg.RPN.NUM_POINTS, 160, 16, cfg.RCNN.NUM_POINTS
    xyz_np = S.scenes(B, N, seed0=400)
    pts = torch.from_numpy(xyz_np).to(DEV)
    rois = np.zeros((B, M, 7), np.float32)
    for b in range(B):
        ctr = xyz_np[b, rng.integers(0, N, M)]                               # centred on real points: non-empty boxes
        rois[b, :, 0:3] = ctr + rng.normal(0, 0.5, (M, 3))
        rois[b, :, 1] += 0.8                                                 # (x, y-bottom, z)
        rois[b, :, 3:6] = rng.uniform([1.2, 1.4, 3.0], [2.2, 2.2, 5.5], (M, 3))
        rois[b, :, 6] = rng.uniform(-np.pi, np.pi, M)
    rois[0, 0] = [0, 2, 35, 6, 80, 90, 0.3]                                  # scene-sized: > 2048 points inside
    rois[0, 1] = [500, 0, 500, 2, 2, 4, 0]                                   # far away: empty
    rois[0, 2, 3:6] = [0.05, 0.05, 12.0]                                     # a needle
    rois[1, 0, 0:3] = [xyz_np[1, :, 0].max(), 1.0, xyz_np[1, :, 2].max()]    # on the corner of the scene
    rois[2, 0, 3:6] = [3.0, 30.0, 30.0]                                      # wide: hundreds to thousands of points
    rois_t = torch.from_numpy(rois).to(DEV)
    feats = torch.from_numpy(rng.standard_normal((B, N, Cf)).astype(np.float32)).to(DEV)
    mask = (torch.rand((B, N), device=DEV) > 0.5).float()
    depth = torch.rand((B, N), device=DEV)
    groups = RU.roipool3d_cuda.point_groups(pts)
    k = groups[0][..., 3].contiguous().view(torch.int32)                      # a permutation of 0..N-1 per scene, coordinates match
    assert torch.equal(torch.sort(k, dim=1).values, torch.arange(N, device=DEV, dtype=torch.int32).expand(B, N))
    assert torch.equal(torch.gather(pts, 1, k.long().unsqueeze(-1).expand(-1, -1, 3)), groups[0][..., :3])
    outs = []
    for g in (None, groups):
        for with_cnt in (False, True):
            pooled = torch.full((B, M, P, 8 + Cf), float("nan"), device=DEV)
            empty = torch.full((B, M), -1, dtype=torch.int32, device=DEV)
            cnt = torch.full((B, M), -1, dtype=torch.int32, device=DEV) if with_cnt else None
            RU.roipool3d_cuda.forward_canonical(pts, rois_t, feats, mask, depth, cfg.RCNN.POOL_EXTRA_WIDTH, pooled, empty, cnt, groups=g)
            outs.append((pooled, empty, cnt))
    for a, bb in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert torch.equal(a[1], bb[1])
        assert torch.equal(torch.nan_to_num(a[0], nan=-777.0), torch.nan_to_num(bb[0], nan=-777.0))
        if a[2] is not None:
            assert torch.equal(a[2], bb[2])
    cnt = outs[3][2]
    assert int(cnt[0, 0]) == P and int(outs[3][1][0, 1]) == 1 and int(cnt.max()) == P and int((cnt > 64).sum()) > 3 and int(outs[3][1].sum()) >= 1


def test_engine_keeps_no_state_from_one_batch_to_the_next():
    """An engine that has already evaluated other batches gives, bit for bit, what a freshly built engine gives.  (Round 2
    cached the packed row list of the RCNN's GroupAll level -- which holds coordinates -- across batches: every batch after
    the first was evaluated with the first batch's SA2 centre coordinates in that level.  The serial-vs-pipelined test could
    not see it, both sides shared the engine.)"""
    C, E, F, S = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer"), pkg("synth")
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, DEV, seed=3)
    a = torch.from_numpy(S.scenes(4, cfg.RPN.NUM_POINTS, seed0=900)).to(DEV)
    b = torch.from_numpy(S.scenes(4, cfg.RPN.NUM_POINTS, seed0=950)).to(DEV)
    used = F.FastPointRCNN(model, cfg)
    E.infer_batch(model, cfg, a, engine=used)
    E.infer_batch(model, cfg, a, engine=used)
    got = E.infer_batch(model, cfg, b, engine=used)
    want = E.infer_batch(model, cfg, b, engine=F.FastPointRCNN(model, cfg))
    for k in ("rois", "rcnn_cls", "rcnn_reg", "boxes", "scores", "num"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["rcnn_reg"], E.infer_batch(model, cfg, a, engine=used)["rcnn_reg"])


@pytest.mark.parametrize("N", [4096, 16384, 10000, 5000, 1000, 40000])
def test_fused_proposal_sort_order_with_ties_and_nans(ext, N):
    """The score sort's total order = (score descending, NaN first, index ascending on ties) == torch's STABLE descending
    sort; argmax over regression bins treats NaN as the largest value like torch.argmax.  Exercised through the fused
    proposal entry with every point in the near band and NMS threshold 1 (nothing suppressed): the RoIs come out in
    exactly that order.  N = 4096: one workgroup per scene (score_sort_kernel); larger N: 4096-key chunks sorted by a
    workgroup each + merge-path rounds (round 3), incl. sizes that are not a power of two (pad keys in the last chunks).
    N = 1000: npad 1024, one workgroup far below a full chunk; N = 40000: npad 65536, four merge rounds, whole chunks of pad keys."""
    rng = np.random.default_rng(3)
    B = 2
    xyz = torch.from_numpy(rng.uniform([-30, 0, 5], [30, 2, 35], (B, N, 3)).astype(np.float32)).to(DEV)
    scores = torch.from_numpy(rng.integers(-3, 4, (B, N)).astype(np.float32)).to(DEV)       # heavy ties
    scores[0, 17] = float("nan"); scores[1, 5] = float("nan"); scores[1, 900] = -float("nan")
    C = pkg("config")
    cfg = C.default_eval_cfg()
    nb = int(cfg.RPN.LOC_SCOPE / cfg.RPN.LOC_BIN_SIZE) * 2
    ch = nb * 4 + 1 + cfg.RPN.NUM_HEAD_BIN * 2 + 3
    reg = torch.from_numpy(rng.standard_normal((B, N, ch)).astype(np.float32)).to(DEV)
    M = 100
    rois = torch.empty((B, M, 7), device=DEV); rs = torch.empty((B, M), device=DEV)
    anchor = [float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32)]
    ext.iou3d.rpn_proposals(xyz, scores, reg, anchor, cfg.RPN.LOC_SCOPE, cfg.RPN.LOC_BIN_SIZE, cfg.RPN.NUM_HEAD_BIN, True,
                            9000, M, 1.0, False, rois, rs)
    key = torch.where(torch.isnan(scores), torch.full_like(scores, float("inf")), scores)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    for b in range(B):
        near = order[b][(xyz[b, order[b], 2] <= 40.0)][:70]          # every point is in the near band here
        got = rs[b, :70]
        want = scores[b, near]
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
        assert bool(torch.isnan(got[0]))                                # the NaN scores lead


def test_final_stage_four_launch_form_keeps_the_best_selected_box(ext):
    """prcnn_rcnn_postprocess with nms_thresh < 0 runs the four-launch form (decode + select, dense NMS, gather; the one-workgroup
    kernel's candidate filter would answer differently there).  Every IoU is >= 0 > threshold, so the best selected box of a scene
    suppresses every other one: num is 1 where any RoI passes the score threshold, slot 0 holds that RoI's decoded box and raw
    score, everything behind is zero; and pred_boxes3d is, bit for bit, the one-workgroup kernel's (the same decode)."""
    from helpers import boxes3d
    cfg = pkg("config").default_eval_cfg()
    R = cfg.RCNN
    rng = np.random.default_rng(52)
    B = 3
    logit = float(np.log(R.SCORE_THRESH / (1.0 - R.SCORE_THRESH)))
    for M in (37, 100, 128):
        rois = torch.from_numpy(np.stack([boxes3d(rng, M) for _ in range(B)])).to(DEV)
        reg = torch.from_numpy((rng.standard_normal((B, M, 46)) * 0.3).astype(np.float32)).to(DEV)
        raw = (rng.standard_normal((B, M)) * 2).astype(np.float32)
        raw[1] = -5.0 - rng.uniform(0, 1, M).astype(np.float32)            # scene 1: nothing above the score threshold
        raw[np.abs(raw - logit) < 0.05] += 0.2                              # no score at the threshold itself
        assert all(len(np.unique(raw[b])) == M for b in range(B))
        cls = torch.from_numpy(raw).to(DEV)
        out = {}
        for thresh in (-1.0, R.NMS_THRESH):
            pred = torch.full((B, M, 7), float("nan"), device=DEV)
            boxes = torch.full((B, M, 7), float("nan"), device=DEV); scores = torch.full((B, M), float("nan"), device=DEV)
            num = torch.full((B,), -9, dtype=torch.int32, device=DEV)
            ext.iou3d.rcnn_postprocess(rois, reg, cls, [float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32)], R.LOC_SCOPE,
                                       R.LOC_BIN_SIZE, R.NUM_HEAD_BIN, R.LOC_Y_BY_BIN, R.LOC_Y_SCOPE, R.LOC_Y_BIN_SIZE, R.SCORE_THRESH,
                                       thresh, pred, boxes, scores, num)
            out[thresh] = (pred, boxes, scores, num)
        pred, boxes, scores, num = out[-1.0]
        assert torch.equal(pred, out[R.NMS_THRESH][0])
        sel = 1.0 / (1.0 + np.exp(-raw.astype(np.float64))) > R.SCORE_THRESH
        assert sel[0].any() and sel[2].any() and not sel[1].any()
        for b in range(B):
            if not sel[b].any():
                assert int(num[b]) == 0 and (boxes[b] == 0).all() and (scores[b] == 0).all()
                continue
            best = int(np.argmax(np.where(sel[b], raw[b], -np.inf)))
            assert int(num[b]) == 1
            assert torch.equal(boxes[b, 0], pred[b, best]) and float(scores[b, 0]) == float(raw[b, best])
            assert (boxes[b, 1:] == 0).all() and (scores[b, 1:] == 0).all()


def test_postprocess_batched_equals_per_scene_reference_order():
    """The batched device tail (masked sort + batched NMS) == the reference's per-scene loop
    (eval_rcnn.py:611-629) run with the blocking drop-in API on the same device tensors."""
    C, E, ku, iu = pkg("config"), pkg("eval_rcnn"), pkg("kitti_utils"), pkg("iou3d_utils")
    cfg = C.default_eval_cfg()
    rng = np.random.default_rng(6)
    B, M = 4, 100
    from helpers import boxes3d
    rois = torch.from_numpy(np.stack([boxes3d(rng, M, xz_scope=((-8, 8), (8, 24))) for _ in range(B)])).to(DEV)
    ret = {"rois": rois, "rcnn_cls": torch.from_numpy(rng.standard_normal((B * M, 1)).astype(np.float32) * 2).to(DEV),
           "rcnn_reg": torch.from_numpy(rng.standard_normal((B * M, 46)).astype(np.float32)).to(DEV)}
    ret["rcnn_cls"][:M] = -5.0     # scene 0: nothing above the score threshold
    det = E.postprocess(cfg, ret, B)
    assert int(det["num"][0]) == 0
    for k in range(B):
        raw = det["raw_scores"][k]
        sel = torch.sigmoid(raw) > cfg.RCNN.SCORE_THRESH
        if sel.sum() == 0:
            continue
        boxes, sc = det["pred_boxes3d"][k][sel], raw[sel]
        keep = iu.nms_gpu(ku.boxes3d_to_bev_torch(boxes), sc, cfg.RCNN.NMS_THRESH)
        n = int(det["num"][k])
        assert n == len(keep)
        assert torch.equal(det["boxes"][k, :n], boxes[keep]) and torch.equal(det["scores"][k, :n], sc[keep])
        assert (det["boxes"][k, n:] == 0).all()


def test_fused_proposal_layer_equals_batched_torch_path():
    """csrc/proposal.hip (decode + score sort + band selection + NMS + assembly) vs the batched torch-op
    formulation of net/proposal_layer.py (itself checked against the reference's per-scene loop in
    tests/test_host_logic.py), incl. a scene with no far points and one with fewer near points than
    the quota."""
    C = pkg("config")
    cfg = C.default_eval_cfg()
    PL = pkg("net.proposal_layer").ProposalLayer(cfg, mode="TEST").to(DEV)
    rng = np.random.default_rng(44)
    B, N = 4, 16384
    xyz = rng.uniform([-40, -1, 0.5], [40, 3, 70], (B, N, 3)).astype(np.float32)
    xyz[1, :, 2] = rng.uniform(0.5, 39.5, N)                 # scene 1: nothing beyond 40 m
    xyz[2, 3000:, 2] = rng.uniform(41, 70, N - 3000)         # scene 2: only 3000 near points
    xyz[3, :, 2] = rng.uniform(100, 120, N)                  # scene 3: neither band -> no proposals
    xyz[3, :50, 2] = rng.uniform(1, 30, 50)                  #          ... except 50 near points
    xyz = torch.from_numpy(xyz).to(DEV)
    reg = torch.from_numpy((rng.standard_normal((B, N, 76)) * 0.5).astype(np.float32)).to(DEV)
    scores = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32)).to(DEV)
    PL.fused = True
    rois_f, sc_f = PL(scores, reg, xyz)
    PL.fused = False
    rois_t, sc_t = PL(scores, reg, xyz)
    torch.cuda.synchronize()
    assert torch.equal(sc_f, sc_t)
    assert torch.equal(rois_f, rois_t), float((rois_f - rois_t).abs().max())
    assert (rois_t[3].abs().sum(-1) > 0).sum() <= 50 and (rois_t[0].abs().sum(-1) > 0).sum() == 100


def test_fused_final_stage_equals_batched_torch_path():
    """prcnn_rcnn_postprocess (decode against the RoIs + threshold + LDS score sort + rotated NMS + assembly)
    vs the batched torch-op formulation of eval_rcnn.postprocess (itself checked against the reference's
    per-scene order above).  Boxes within 1e-5 (the torch path rotates through a batched matmul whose
    contraction is the library's), selection identical; both LOC_Y_BY_BIN settings; a scene with nothing
    above the threshold."""
    C, E = pkg("config"), pkg("eval_rcnn")
    rng = np.random.default_rng(46)
    for y_by_bin, M in ((False, 100), (True, 100), (False, 128), (True, 37)):          # (round 4: the one-workgroup kernel takes any M <= 128)
        cfg = C.default_eval_cfg()
        cfg.RCNN.LOC_Y_BY_BIN = y_by_bin
        B = 5
        ch = 4 * 6 + (2 * 4 if y_by_bin else 1) + 2 * 9 + 3
        rois = np.zeros((B, M, 7), np.float32)
        centres = rng.uniform([-20, 1, 5], [20, 2, 60], (B, 12, 3))
        for b in range(B):
            which = rng.integers(0, 12, M)
            rois[b, :, :3] = centres[b, which] + rng.normal(0, 0.4, (M, 3))
            rois[b, :, 3:6] = [1.5, 1.6, 3.9] + rng.normal(0, 0.05, (M, 3))
            rois[b, :, 6] = rng.uniform(-np.pi, np.pi, M)
        reg = (rng.standard_normal((B, M, ch)) * 0.3).astype(np.float32)
        cls = (rng.standard_normal((B, M, 1)) * 2).astype(np.float32)
        cls[3] = -5.0                                                 # scene 3: nothing passes the threshold
        cls[4, 10:] = -5.0                                            # scene 4: ten candidates
        ret = {"rois": torch.from_numpy(rois).to(DEV), "rcnn_reg": torch.from_numpy(reg).to(DEV).view(B * M, ch),
               "rcnn_cls": torch.from_numpy(cls).to(DEV).view(B * M, 1)}
        pkg("runners").FUSED_POSTPROCESS = True
        f = E.postprocess(cfg, ret, B)
        pkg("runners").FUSED_POSTPROCESS = False
        try:
            t = E.postprocess(cfg, ret, B)
        finally:
            pkg("runners").FUSED_POSTPROCESS = True
        torch.cuda.synchronize()
        assert (f["pred_boxes3d"] - t["pred_boxes3d"]).abs().max().item() < 1e-5
        assert torch.equal(f["num"], t["num"]), (f["num"], t["num"])
        assert int(f["num"][3]) == 0 and 0 < int(f["num"][4]) <= 10 and int(f["num"][0]) > 5
        assert torch.equal(f["scores"], t["scores"])
        assert (f["boxes"] - t["boxes"]).abs().max().item() < 1e-5


def test_final_stage_with_every_pair_a_candidate():
    """The one-workgroup final stage when EVERY pair of boxes is a candidate (128 boxes jittered around one spot: 8128 pairs on the
    compacted list, its capacity), when boxes are exact copies of one another (score ties broken by index, IoU exactly 1), with
    degenerate (zero-width) boxes among them, and with one selected box: same survivors as the batched torch path."""
    C, E = pkg("config"), pkg("eval_rcnn")
    rng = np.random.default_rng(48)
    cfg = C.default_eval_cfg()
    B, M = 4, 128
    ch = 4 * 6 + 1 + 2 * 9 + 3
    rois = np.zeros((B, M, 7), np.float32)
    rois[:, :, :3] = np.array([3.0, 1.5, 20.0], np.float32) + rng.normal(0, 0.3, (B, M, 3))
    rois[:, :, 3:6] = [1.5, 1.6, 3.9]
    rois[:, :, 6] = rng.uniform(-np.pi, np.pi, (B, M))
    reg = (rng.standard_normal((B, M, ch)) * 0.05).astype(np.float32)
    cls = (rng.standard_normal((B, M, 1)) * 0.5 + 2.0).astype(np.float32)          # everything passes the threshold
    rois[1, 1::2] = rois[1, 0::2]; reg[1, 1::2] = reg[1, 0::2]; cls[1, 1::2] = cls[1, 0::2]      # scene 1: pairs of exact copies
    reg[2, :, -3:-1] = -1.0                                                        # scene 2: h = w = 0 for every box (zero-area BEV boxes)
    cls[3, 1:] = -6.0                                                              # scene 3: one box
    ret = {"rois": torch.from_numpy(rois).to(DEV), "rcnn_reg": torch.from_numpy(reg).to(DEV).view(B * M, ch),
           "rcnn_cls": torch.from_numpy(cls).to(DEV).view(B * M, 1)}
    pkg("runners").FUSED_POSTPROCESS = True
    f = E.postprocess(cfg, ret, B)
    pkg("runners").FUSED_POSTPROCESS = False
    try:
        t = E.postprocess(cfg, ret, B)
    finally:
        pkg("runners").FUSED_POSTPROCESS = True
    torch.cuda.synchronize()
    assert torch.equal(f["num"], t["num"]), (f["num"], t["num"])
    assert int(f["num"][3]) == 1 and int(f["num"][0]) >= 1 and int(f["num"][1]) <= M // 2
    assert torch.equal(f["scores"], t["scores"])
    assert (f["boxes"] - t["boxes"]).abs().max().item() < 1e-5
    assert (f["pred_boxes3d"] - t["pred_boxes3d"]).abs().max().item() < 1e-5


def test_eval_scenes_writes_kitti_result_files(tmp_path):
    """Harness loop on the GPU (pipelined runner) over a few synthetic scenes: one KITTI result file per
    scene (empty file when nothing survives), 16 fields per line, and the packed table agrees with them.
    Scenes 80 and 81 are the two scenes of the REFERENCE-model fixture g8 (make_golden.py: helpers.scenes(2, 2048,
    seed0=80)): their detections must be the reference's."""
    E, K = pkg("eval_rcnn"), pkg("kitti_io")
    model, cfg, g = tiny_model(DEV)
    src = K.SyntheticSource(cfg, 5)
    src.ids = [80, 81, 82, 83, 84]
    assert np.array_equal(src.load(80)[0], g["pts"][0]) and np.array_equal(src.load(81)[0], g["pts"][1])
    out = tmp_path / "final_result" / "data"
    table, counts = E.eval_scenes(model, cfg, DEV, src, src.ids, batch_size=2, output_dir=str(out))
    assert table.shape == (5, cfg.TEST.RPN_POST_NMS_TOP_N, 9) and counts.shape == (5,)
    for k, sid in enumerate(src.ids):
        assert int(table[k, 0, 8]) == sid
        lines = [l for l in open(out / ("%06d.txt" % sid)).read().split("\n") if l]
        assert len(lines) <= int(counts[k])
        for l in lines:
            f = l.split()
            assert len(f) == 16 and f[0] == "Car"
    assert int(counts.sum()) > 0
    for k in (0, 1):
        n = int(g["final_num"][k])
        assert int(counts[k]) == n
        np.testing.assert_allclose(table[k, :n, 0:7].numpy(), g["final_boxes"][k, :n], rtol=0, atol=1e-4)
        np.testing.assert_allclose(table[k, :n, 7].numpy(), g["final_scores"][k, :n], rtol=0, atol=1e-4)


def test_sharded_eval_tail_computes_ap_on_gpu():
    """eval_scenes -> gathered table -> AP text with the rotated IoU on the GPU (random weights: the number is
    meaningless, the plumbing is what is checked), and perfect detections score 100 through the HIP kernel."""
    import test_kitti_eval as TK
    E, K = pkg("eval_rcnn"), pkg("kitti_io")
    model, cfg, g = tiny_model(DEV)
    src = K.SyntheticSource(cfg, 4)
    table, counts = E.eval_scenes(model, cfg, DEV, src, src.ids, batch_size=2)
    text, ret = E.evaluate_detections(table, counts, src)
    assert text.startswith("Car AP@0.70, 0.70, 0.70:") and "3d   AP:" in text and np.isfinite(float(ret["Car_3d_moderate"]))
    E2, src2, table2, counts2 = TK.synthetic_perfect_table(16)
    _, ret2 = E2.evaluate_detections(table2, counts2, src2)
    for k in ("Car_3d_easy", "Car_3d_moderate", "Car_3d_hard", "Car_bev_moderate"):
        assert abs(float(ret2[k]) - 100.0) < 1e-9, (k, ret2[k])


def test_reference_python_runs_on_dropin_modules():
    """Drop-in check at the extension boundary: a caller written against the REFERENCE module names
    and calling conventions (zero-filled idx, transposes, in-place subtract, cat -- the sequence of
    pointnet2_utils.py:241-264) gets the same tensor as the fused path."""
    import sys
    p = pkg()
    if p.DROPIN_DIR not in sys.path:
        sys.path.insert(0, p.DROPIN_DIR)
    import pointnet2_cuda as pointnet2
    xyz = torch.from_numpy(pkg("synth").scenes(2, 4096, seed0=9)).to(DEV)
    new_xyz = xyz[:, :512].contiguous()
    feats = torch.randn((2, 32, 4096), device=DEV)
    idx = torch.zeros((2, 512, 16), dtype=torch.int32, device=DEV)
    pointnet2.ball_query_wrapper(2, 4096, 512, 0.6, 16, new_xyz, xyz, idx)
    xyz_t = xyz.transpose(1, 2).contiguous()
    gx = torch.empty((2, 3, 512, 16), device=DEV)
    pointnet2.group_points_wrapper(2, 3, 4096, 512, 16, xyz_t, idx, gx)
    gx -= new_xyz.transpose(1, 2).unsqueeze(-1)
    gf = torch.empty((2, 32, 512, 16), device=DEV)
    pointnet2.group_points_wrapper(2, 32, 4096, 512, 16, feats, idx, gf)
    composed = torch.cat([gx, gf], dim=1)
    fused = pkg("pointnet2.pointnet2_utils").QueryAndGroup(0.6, 16)(xyz, new_xyz, feats)
    assert torch.equal(composed, fused)
