"""-m gpu: the "live rows" form of the RCNN's RoI geometry (prcnn_rcnn_roi_geometry_live, prcnn_pooled_rows_src_live): of SA level 1
only what SA level 2 reads.  A level-1 centre is live iff a row of the level-2 list names it; a pooled point is live iff a row of the kept
level-1 list names it.

  A  the lists: the expected sets and lists are made in numpy from the index tensors and maps of the EXISTING entry on the same clouds
     (tests/row_lists.py is the definition of a list); lists 2 and 3 are the existing ones, list 1 / the centre rows / the pooled-row
     list are exactly the live subsets, per cloud (the order of the clouds in a list is the counter's), in both forms of a list; the rows
     that fill a cloud's last tile repeat a listed row.
  B  the engine with the switch on and off: head outputs and detections bit for bit.
Every comparison is exact; there is no tolerance in this file."""
import importlib

import numpy as np
import pytest
import torch

import row_lists as R
from test_gpu_row_lists import assert_list_by_cloud, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "3d_adapt_auto_driving_amd"
N, M1, M2, NS = 512, 128, 32, 64
R1, R2 = 0.2, 0.4                                   # default.yaml: RCNN.SA_CONFIG.RADIUS[0:2], NSAMPLE 64
LIMITS = (1, 2, 31, 33, 64, 200, 512, 512)


def live_clouds():
    """eight RoI clouds of 512 pooled rows, rows k >= limit copies of row k % limit:
      limit 1, 2      one point, two points 0.3 m apart
      limit 31, 33    points spread over a 4 x 2 x 1.5 m box: fewer distinct points than level 2 samples -- every centre is sampled again
      limit 64        a 4 x 4 x 4 lattice with spacing 0.5 m > r2: every ball holds its centre alone
      limit 200       two clusters of 100 points, 0.3 m wide, 5 m apart
      limit 512       all points within 0.1 m: every ball is cut at nsample
      limit 512       the box again, full"""
    rng = np.random.default_rng(8)
    box = np.float32([4.0, 2.0, 1.5])
    d = []
    d.append(np.float32([[0.3, -0.2, 0.1]]))
    d.append(np.float32([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0]]))
    d.append((rng.random((31, 3)) * box).astype(np.float32))
    d.append((rng.random((33, 3)) * box).astype(np.float32))
    g = np.arange(4, dtype=np.float32) * 0.5
    d.append(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(64)])
    two = (rng.random((200, 3)) * 0.3).astype(np.float32)
    two[100:, 0] += 5.0
    d.append(two[rng.permutation(200)])
    d.append((rng.random((512, 3)) * 0.1).astype(np.float32))
    d.append((rng.random((512, 3)) * box).astype(np.float32))
    assert tuple(len(p) for p in d) == LIMITS
    xyz = np.stack([p[np.arange(N) % len(p)] for p in d]).astype(np.float32)
    return xyz, np.asarray(LIMITS, np.int32)


def live_definition(xyz, limit, new1, idx1, rep1, new2, idx2, rep2):
    """from the index tensors and maps of the full chain -> per cloud (used1, used0, list 1 of the live centres), and the full lists 2, 3"""
    b = len(limit)
    l1 = R.row_list(idx1, xyz, new1, limit=limit, crep=rep1)
    l2 = R.row_list(idx2, new1, new2, rep=rep1, crep=rep2)
    l3 = R.row_list(np.tile(np.arange(M2, dtype=np.int32), (b, 1, 1)), new2, np.zeros((b, 1, 3), np.float32), rep=rep2)
    used1, used0, live1 = [], [], []
    for c in range(b):
        u1 = np.unique(l2[c][0] & 0xffff).astype(np.int64)                 # the level-1 centres that level 2's rows name
        info, dxyz, cnt = l1[c]
        keep = np.isin(info >> 16, u1)
        rows = R.CloudRows((info[keep], dxyz[keep], np.where(np.isin(np.arange(M1), u1), cnt, 0)))
        rows.pad = (rows[0][-1], rows[1][-1].copy())                        # a cloud's last tile is filled with its last listed row
        used1.append(u1)
        used0.append(np.unique(rows[0] & 0xffff).astype(np.int64))
        live1.append(rows)
    return used1, used0, live1, l1, l2, l3


def rows_by_cloud(pk, b):
    """a list whose rows carry their cloud -> per cloud (centre << 16 | point as row_lists writes it, rowdxyz bits); blocks are contiguous"""
    assert pk.tilecloud is None
    n = int(pk.hdr[1])
    info = pk.rowinfo[:n].cpu().numpy().view(np.uint32).astype(np.int64)
    dx = pk.rowdxyz[:n].cpu().numpy().view(np.uint32)
    out = []
    for c in range(b):
        sel = np.nonzero(info >> 16 == c)[0]
        assert len(sel) > 0 and (np.diff(sel) == 1).all(), c
        w = info[sel] & 0xffff
        out.append(((((w >> 9) << 16) | (w & 0x1ff)).astype(np.uint32), dx[sel]))
    assert sum(len(i) for i, _ in out) == n
    return out


def assert_rows(got, want, what):
    for c, ((gi, gd), w) in enumerate(zip(got, want)):
        assert np.array_equal(gi, w[0]), (what, c, "rowinfo")
        assert np.array_equal(gd, w[1].view(np.uint32)), (what, c, "rowdxyz")


def test_live_lists_are_the_live_subsets_of_the_full_lists(ext):
    P = ext.pointnet2
    xyz, limit = live_clouds()
    b = len(limit)
    X, L = torch.from_numpy(xyz).to(DEV), torch.from_numpy(limit).to(DEV)
    full = P.rcnn_roi_geometry_packs_wrapper(X, L, M1, R1, NS, M2, R2, NS)
    new1, idx1, rep1, new2, idx2, rep2 = (t.cpu().numpy() for t in full[:6])
    used1, used0, live1, l1, l2, l3 = live_definition(xyz, limit, new1, idx1, rep1, new2, idx2, rep2)
    # what the clouds were built for, on the numpy side, before the new entry runs
    distinct = [np.nonzero(rep1[c] == np.arange(M1))[0] for c in range(b)]
    kept = [len(u) for u in used1]
    assert all(np.isin(u, dc).all() for u, dc in zip(used1, distinct))
    assert any(k == len(dc) for k, dc in zip(kept, distinct)) and any(k < len(dc) for k, dc in zip(kept, distinct)), (kept, [len(dc) for dc in distinct])
    assert all(0 in u for u in used1) and all(0 in u for u in used0)
    lattice, tight, two = LIMITS.index(64), LIMITS.index(512), LIMITS.index(200)
    assert (l1[lattice][2][distinct[lattice]] == 1).all() and (l2[lattice][2][rep2[lattice] == np.arange(M2)] == 1).all()    # balls of one
    assert (l1[tight][2][distinct[tight]] == NS).all() and kept[tight] == NS < len(distinct[tight])                          # balls cut at nsample
    assert len(distinct[two]) >= kept[two] > 2 and len(np.unique(new1[two][used1[two], 0] > 2.5)) == 2                      # both clusters
    assert any(len(u0) < min(int(limit[c]), N) for c, u0 in enumerate(used0))            # ... and pooled rows nobody reads

    # ---- with a tilecloud: per cloud its tiles, the last one filled with the cloud's last listed row
    got = P.rcnn_roi_geometry_live_wrapper(X, L, M1, R1, NS, M2, R2, NS)
    assert len(got) == 9 and got[1].device.type == "meta" and got[4].device.type == "meta"
    for k in (0, 2, 3, 5):
        assert torch.equal(got[k], full[k]), k
    h1 = host(got[6])
    assert_list_by_cloud(h1, live1, "level 1, live")
    assert_list_by_cloud(host(got[7]), l2, "level 2")
    for c in range(b):                                                                  # (no padding row names a centre or a point outside the live sets)
        t = np.nonzero(h1["tilecloud"] == c)[0]
        pad = h1["info"].reshape(-1, 64)[t].reshape(-1)[len(live1[c][0]):].astype(np.int64)
        assert np.isin(pad >> 16, used1[c]).all() and np.isin(pad & 0xffff, used0[c]).all(), c
    u0 = got[8].cpu().numpy().view(np.uint32)
    assert u0.shape == (b, N // 32)
    for c in range(b):
        bit = (u0[c][:, None] >> np.arange(32, dtype=np.uint32)[None]) & 1             # word k >> 5, bit k & 31
        assert np.array_equal(np.nonzero(bit.reshape(-1))[0], used0[c]), c

    # ---- rows that carry their cloud, the GroupAll list and the centre rows; pre-zeroed headers as the engine passes them
    z = [torch.zeros(4, dtype=torch.int32, device=DEV) for _ in range(4)]
    got = P.rcnn_roi_geometry_live_wrapper(X, L, M1, R1, NS, M2, R2, NS, z[0], z[1], True, z[2], True, z[3], True)
    assert len(got) == 11
    ref = P.rcnn_roi_geometry_packs_wrapper(X, L, M1, R1, NS, M2, R2, NS, None, None, False, True, None, True, None, True)
    assert_rows(rows_by_cloud(got[6], b), live1, "level 1, live (row-carried)")
    for lvl, want in ((7, l2), (8, l3)):
        assert_rows(rows_by_cloud(got[lvl], b), want, lvl)
        for (gi, gd), (ri, rd) in zip(rows_by_cloud(got[lvl], b), rows_by_cloud(ref[lvl], b)):        # ... the existing entry's
            assert np.array_equal(gi, ri) and np.array_equal(gd, rd), lvl
    rowmap, hdr = got[9]
    rows = rowmap[:int(hdr[1])].cpu().numpy().astype(np.int64)
    assert len(rows) == sum(kept)
    for c in range(b):
        sel = np.nonzero(rows // M1 == c)[0]
        assert (np.diff(sel) == 1).all() and np.array_equal(rows[sel] % M1, used1[c]), c
    assert torch.equal(got[10], got[10].new_tensor(u0.view(np.int32)))

    # ---- the pooled rows that are left, each with the feature row it names
    src = torch.from_numpy(np.random.default_rng(1).integers(-1, 1 << 20, b * N).astype(np.int32)).to(DEV)
    for hz in (None, torch.zeros(4, dtype=torch.int32, device=DEV)):
        rowmap, hdr, featmap = P.pooled_rows_src_live_wrapper(L, N, src, got[10], *(() if hz is None else (hz,)))
        n = int(hdr[1])
        rows = rowmap[:n].cpu().numpy().astype(np.int64)
        assert n == sum(len(u) for u in used0)
        for c in range(b):
            sel = np.nonzero(rows // N == c)[0]
            assert (np.diff(sel) == 1).all() and np.array_equal(rows[sel] % N, used0[c]), c
        assert np.array_equal(featmap[:n].cpu().numpy(), src.cpu().numpy()[rows])
    with pytest.raises(ValueError):
        P.pooled_rows_src_live_wrapper(L, N, src, got[10][:-1].contiguous())


def test_engine_outputs_do_not_depend_on_the_live_rows_switch(monkeypatch):
    """FastPointRCNN.forward on two uniform and two LiDAR-shaped scenes, level 1 cut down to what level 2 reads (the default) against
    every distinct row: rcnn_cls, rcnn_reg and the detections, bit for bit; the default run took the new entries, the other did not"""
    C, E, S, F = (importlib.import_module(PKG + "." + m) for m in ("config", "eval_rcnn", "synth", "net.fast_infer"))
    dev = torch.device("cuda", 0)
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, dev, seed=0)
    batches = [torch.from_numpy(make(2, cfg.RPN.NUM_POINTS, seed0=810 + 2 * k)).to(dev) for k, make in enumerate((S.scenes, S.lidar_scenes))]
    pn = F.pu.pointnet2
    calls = {"live": 0, "rows": 0}
    real_geo, real_rows = pn.rcnn_roi_geometry_live_wrapper, pn.pooled_rows_src_live_wrapper

    def counted(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    monkeypatch.setattr(pn, "rcnn_roi_geometry_live_wrapper", counted("live", real_geo))
    monkeypatch.setattr(pn, "pooled_rows_src_live_wrapper", counted("rows", real_rows))

    def run():
        eng = F.FastPointRCNN(model, cfg)
        out = [E.infer_batch(model, cfg, x, engine=eng) for x in batches]
        torch.cuda.synchronize()
        return out
    monkeypatch.setattr(F, "USE_LIVE_ROWS", True)
    got = run()
    assert calls == {"live": len(batches), "rows": len(batches)}
    monkeypatch.setattr(F, "USE_LIVE_ROWS", False)
    want = run()
    assert calls == {"live": len(batches), "rows": len(batches)}
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("rcnn_cls", "rcnn_reg", "boxes", "scores", "num"):
            assert torch.equal(g[k], w[k]), (i, k)
    assert sum(int(w["num"].sum()) for w in want) > 0
