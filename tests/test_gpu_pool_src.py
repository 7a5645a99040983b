"""-m gpu: RoI pooling that copies no features.  The pooled rows NAME their points (prcnn_roipool3d_canonical_src: rows of 8 floats and
`src`, each row's row of the RPN's feature matrix), the list of distinct rows hands the names on (prcnn_pooled_rows_src: featmap) and the
RCNN entrance gathers the features where they are (prcnn_rcnn_point_mlp_rows_src).  Each link against the copying entry on the same
inputs, `src` against a numpy definition row for row, and the engine through the new wiring against the copying one under both runners.
Every comparison is exact (floats as their bit patterns); there is no tolerance in this file."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "3d_adapt_auto_driving_amd"
EXTRA = 1.0                     # pool_extra_width: every box side grows by 2, the bottom drops by 1


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
B, N, M, S, C = 2, 256, 4, 64, 128
HOLD = ((0, 5, 64, 100), (100, 64, 0, 5))          # points inside box m of scene b: empty / wrap-around / exactly S / more than S


def pool_case():
    """hand-placed clouds: box m of a scene sits at x = 10 m (1 x 1 x 1 m, enlarged to 3 x 3 x 3), its points within 0.9 m of the centre
    line -- inside at any heading, far from every face -- the rest of the cloud 100 m away; the cloud's index order is shuffled"""
    rng = np.random.default_rng(11)
    xyz = np.zeros((B, N, 3), np.float32)
    rois = np.zeros((B, M, 7), np.float32)
    for b in range(B):
        pts = []
        for m in range(M):
            rois[b, m] = [10.0 * m, 0.0, 2.0 * b, 1.0, 1.0, 1.0, 0.3 + 0.7 * m - 1.1 * b]
            p = rng.uniform(-0.9, 0.9, (HOLD[b][m], 3)).astype(np.float32)
            pts.append(p + np.float32([10.0 * m, -0.5, 2.0 * b]))          # (the enlarged box spans y in [-2, 1])
        rest = N - sum(HOLD[b])
        pts.append(rng.uniform(-5, 5, (rest, 3)).astype(np.float32) + np.float32([-100.0, 0.0, 0.0]))
        xyz[b] = np.concatenate(pts)[rng.permutation(N)]
    feats = rng.standard_normal((B, N, C)).astype(np.float32)
    mask = (rng.random((B, N)) > 0.5).astype(np.float32)
    depth = rng.standard_normal((B, N)).astype(np.float32)
    return xyz, rois, feats, mask, depth


def src_definition(xyz, rois):
    """the first S indices inside the enlarged box in ascending order, then wrapped; -1 everywhere for an empty box.  -> (src, cnt)"""
    src = np.full((B, M, S), -1, np.int32)
    cnt = np.zeros((B, M), np.int32)
    for b in range(B):
        for m in range(M):
            x, yb, z, h, w, l, ry = rois[b, m].astype(np.float64)
            h, w, l, yb = h + 2 * EXTRA, w + 2 * EXTRA, l + 2 * EXTRA, yb + EXTRA
            d = xyz[b].astype(np.float64) - [x, yb - h / 2, z]
            xr = d[:, 0] * np.cos(ry) - d[:, 2] * np.sin(ry)
            zr = d[:, 0] * np.sin(ry) + d[:, 2] * np.cos(ry)
            inside = np.nonzero((np.abs(d[:, 1]) <= h / 2) & (np.abs(xr) <= l / 2) & (np.abs(zr) <= w / 2))[0][:S]
            cnt[b, m] = len(inside)
            if len(inside):
                src[b, m] = b * N + inside[np.arange(S) % len(inside)]
    return src, cnt


@pytest.mark.parametrize("grouped", [False, True])
def test_pooling_names_the_points_the_copying_form_copies(ext, grouped):
    xyz, rois, feats, mask, depth = pool_case()
    want_src, want_cnt = src_definition(xyz, rois)
    assert want_cnt.tolist() == [[min(h, S) for h in hs] for hs in HOLD]                        # the case holds what it says
    rp = ext.roipool3d
    txyz, trois, tfeats, tmask, tdepth = T(xyz), T(rois), T(feats), T(mask), T(depth)
    groups = rp.point_groups(txyz) if grouped else None
    nanf = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    # the copying entry
    pooled, xo0 = nanf(B, M, S, 8 + C), nanf(B, M, S, 3)
    empty0, cnt0 = (torch.full((B, M), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    rp.forward_canonical(txyz, trois, tfeats, tmask, tdepth, EXTRA, pooled, empty0, cnt0, groups, xo0)
    # the naming entry
    rows, xo1 = nanf(B, M, S, 8), nanf(B, M, S, 3)
    src = torch.full((B, M, S), -7, dtype=torch.int32, device=DEV)
    empty1, cnt1 = (torch.full((B, M), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    rp.forward_canonical_src(txyz, trois, tmask, tdepth, EXTRA, rows, src, empty1, cnt1, groups, xo1)
    torch.cuda.synchronize()
    assert torch.equal(bits(rows), bits(pooled[..., :8])), "slim rows differ from columns 0..7 of the copied rows"
    assert torch.equal(cnt1.cpu(), cnt0.cpu()) and torch.equal(empty1.cpu(), empty0.cpu()) and torch.equal(bits(xo1), bits(xo0))
    assert np.array_equal(cnt1.cpu().numpy(), np.maximum(want_cnt, 1)) and np.array_equal(empty1.cpu().numpy(), (want_cnt == 0).astype(np.int32))
    got_src = src.cpu().numpy()
    assert np.array_equal(got_src, want_src), "src differs from its definition"
    # wrap-around rows repeat row s % cnt; an empty box names nothing
    for b in range(B):
        for m in range(M):
            c = int(want_cnt[b, m])
            if c == 0:
                assert (got_src[b, m] == -1).all()
            else:
                assert np.array_equal(got_src[b, m], got_src[b, m][np.arange(S) % c])
    # every row below the copy's feat_rows (= S here: the next multiple of 64 above any count): the named row IS the copied one
    flat = np.concatenate([feats.reshape(B * N, C), np.zeros((1, C), np.float32)])             # (index -1: the zero row)
    named = flat[got_src.reshape(-1)].reshape(B, M, S, C)
    assert np.array_equal(named.view(np.int32), pooled[..., 8:].cpu().numpy().view(np.int32)), "feats[src[row]] differs from the copied features"
    with pytest.raises(Exception):
        rp.forward_canonical_src(txyz, trois, tmask, tdepth, EXTRA, rows, src.view(B, M * S), empty1, cnt1, groups, xo1)


# ---- list --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,cnt", [
    ("a tile boundary inside a RoI", [40, 40, 40, 40, 40, 40]),
    ("a tile boundary between RoIs of two scenes", [64, 64, 64, 10, 0, 5]),
    ("a tile boundary on an empty box", [64, 0, 63, 0, 64, 1]),
])
def test_list_hands_on_the_feature_row_of_every_listed_row(ext, what, cnt):
    """two scenes of three RoIs of 64 rows; whichever order the device counter hands the clouds out in, entry e of featmap is src of the
    row entry e of rowmap names, and the list is the definition's"""
    P = 64
    rng = np.random.default_rng(len(what))
    src = rng.integers(0, 2 * 256, (len(cnt), P)).astype(np.int32)
    src[np.array(cnt) == 0] = -1
    tcnt, tsrc = T(np.array(cnt, np.int32)), T(src.reshape(-1))
    for hdr in (None, torch.zeros(4, dtype=torch.int32, device=DEV)):
        rowmap, h, featmap = ext.pointnet2.pooled_rows_src_wrapper(tcnt, P, tsrc, *(() if hdr is None else (hdr,)))
        n = int(h[1])
        want_rows = np.concatenate([np.arange(max(c, 1)) + P * i for i, c in enumerate(cnt)])
        got_rows = rowmap[:n].cpu().numpy()
        assert n == len(want_rows) and np.array_equal(np.sort(got_rows), want_rows), what
        assert np.array_equal(featmap[:n].cpu().numpy(), src.reshape(-1)[got_rows]), what
        # the plain list of the same counts holds the same rows
        plain = ext.pointnet2.pooled_rows_wrapper(tcnt, P)
        assert int(plain[1][1]) == n and np.array_equal(np.sort(plain[0][:n].cpu().numpy()), want_rows)
    with pytest.raises(Exception):
        ext.pointnet2.pooled_rows_src_wrapper(tcnt, P, tsrc[:-1].contiguous())


# ---- entrance ----------------------------------------------------------------------------------------------------------------------
_ENTRANCE = {}


def entrance_case():
    """256 pooled rows, a feature matrix of two scenes x 150 points with a NaN row (row 0: also what a negative entry's address falls
    on), an inf row, and the chain's weights"""
    if not _ENTRANCE:
        rng = np.random.default_rng(73)
        R, F = 256, 300
        head = rng.standard_normal((R, 8)).astype(np.float32)
        head[:, 5:8] = 0
        feats = rng.standard_normal((F, 128)).astype(np.float32)
        feats[0, 17] = np.nan
        feats[200, 5] = np.inf
        W = lambda *sh: (rng.standard_normal(sh) / np.sqrt(sh[0])).astype(np.float32)
        wu1 = W(8, 128); wu1[5:] = 0
        ws = [wu1, rng.standard_normal(128).astype(np.float32) * 0.1]
        for k in (128, 256, 128):
            ws += [W(k, 128), rng.standard_normal(128).astype(np.float32) * 0.1]
        _ENTRANCE.update(R=R, F=F, head=head, feats=feats, ws=[T(w) for w in ws])
    return _ENTRANCE


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_entrance_gathering_at_the_source_equals_the_entrance_over_copied_rows(ext, n):
    c = entrance_case()
    R, F, head, feats = c["R"], c["F"], c["head"], c["feats"]
    rng = np.random.default_rng(n)
    rowmap = rng.permutation(R)[:n].astype(np.int32)
    featmap = rng.integers(1, F, n).astype(np.int32)                       # rows of both scenes side by side in a tile
    if n > 1:
        featmap[0], featmap[1] = 0, 200                                    # the NaN row, the inf row
    featmap[n // 2] = -1                                                   # the listed row of an empty box
    copied = np.full((R, 136), np.nan, np.float32)                         # (rows that are not listed: never read)
    copied[:, :8] = head
    copied[rowmap, 8:] = np.where((featmap >= 0)[:, None], feats[np.maximum(featmap, 0)], np.float32(0))
    hdr = T(np.array([0, n, 0, 0], np.int32))
    p_old, p_new = (torch.full((R, 128), float("nan"), device=DEV) for _ in range(2))
    ext.pointnet2.rcnn_point_mlp_rows_wrapper(T(copied), 8, *c["ws"], p_old, (T(rowmap), hdr))
    ext.pointnet2.rcnn_point_mlp_rows_src_wrapper(T(head), T(feats), *c["ws"], p_new, (T(rowmap), hdr, T(featmap)))
    torch.cuda.synchronize()
    assert torch.equal(bits(p_new), bits(p_old)), "P differs between gathering at the source and the copied rows (list of %d)" % n
    listed = torch.zeros(R, dtype=torch.bool); listed[torch.from_numpy(rowmap).long()] = True
    got = p_new.cpu()
    assert torch.isnan(got[~listed]).all()                                 # rows that are not listed are left as they were
    # (the NaN and the inf reach T1 as they are -- the bit-for-bit equality above is over them too; what P shows of them is the chain's
    # business: its ReLU is an fmaxf, which drops a NaN.)  The zero row of the empty box took nothing from row 0, whose address it was given:
    clean = listed.clone(); clean[torch.from_numpy(rowmap[featmap == 0]).long()] = False; clean[torch.from_numpy(rowmap[featmap == 200]).long()] = False
    assert torch.isfinite(got[clean]).all()


# ---- engine ------------------------------------------------------------------------------------------------------------------------
KEYS = ("boxes", "scores", "num", "pred_boxes3d", "rois", "rcnn_cls", "rcnn_reg")


def _run(runner, batches):
    outs = []

    def take(det):
        if det is not None:
            with torch.cuda.stream(det["stream"]):
                outs.append({k: det[k].clone() for k in KEYS})
    for i, b in enumerate(batches):
        take(runner.submit(b, batches[i + 1:i + 1 + runner.depth]))
    while True:
        det = runner.flush()
        if det is None:
            break
        take(det)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("runner", ["PipelinedRunner", "GraphedRunner"])
def test_engine_detections_are_those_of_the_copying_form(runner, monkeypatch):
    """batches of two scenes (uniform and LiDAR-shaped in turn) through the eager runner and through graph replay: the pooled rows
    naming their features (the default) against `_pool_canonical` on the copying entries, every detection tensor bit for bit"""
    C, E, S, F = (importlib.import_module(PKG + "." + m) for m in ("config", "eval_rcnn", "synth", "net.fast_infer"))
    dev = torch.device("cuda", 0)
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, dev, seed=0)
    batches = [torch.from_numpy((S.lidar_scenes if k % 2 else S.scenes)(2, cfg.RPN.NUM_POINTS, seed0=700 + 2 * k)).to(dev) for k in range(5)]
    calls = {"src": 0, "copy": 0}
    ru = importlib.import_module(PKG + ".roipool3d_utils")
    real_src, real_copy = ru.roipool3d_cuda.forward_canonical_src, ru.roipool3d_cuda.forward_canonical

    def counted(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    monkeypatch.setattr(ru.roipool3d_cuda, "forward_canonical_src", counted("src", real_src))
    monkeypatch.setattr(ru.roipool3d_cuda, "forward_canonical", counted("copy", real_copy))
    assert F.USE_POOL_BY_NAME
    first = getattr(E, runner)(model, cfg, dev)
    got = _run(first, batches)
    assert calls["src"] > 0 and calls["copy"] == 0                         # the product path took the new entries ...
    assert runner != "GraphedRunner" or first.captures > 0                 # ... inside captured graphs, where that is the runner
    monkeypatch.setattr(F, "USE_POOL_BY_NAME", False)
    want = _run(getattr(E, runner)(model, cfg, dev), batches)
    assert calls["copy"] > 0                                               # ... and the reference run the copying ones
    assert len(got) == len(want) == len(batches)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert torch.equal(bits(g[k].float()) if g[k].is_floating_point() else g[k].cpu(),
                               bits(w[k].float()) if w[k].is_floating_point() else w[k].cpu()), "batch %d: %s" % (i, k)
    assert sum(int(w["num"].sum()) for w in want) > 0
