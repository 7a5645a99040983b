"""CPU tests of the ORACLE itself: (1) against independent numpy / float64 implementations written
from the operators' definitions, (2) against the committed golden vectors (regression pins),
(3) against outputs of the reference's own compiled CPU code (g5)."""
import os

import numpy as np

from helpers import scenes, bev_boxes

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


# ---------------------------------------------------------------- independent references
def ball_query_np(r, ns, xyz, new):
    out = np.zeros((xyz.shape[0], new.shape[1], ns), np.int32)
    r2 = np.float32(r) * np.float32(r)
    for b in range(xyz.shape[0]):
        for p in range(new.shape[1]):
            d = new[b, p][None, :] - xyz[b]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]   # f32, left to right
            hit = np.nonzero(d2 < r2)[0][:ns]
            if len(hit):
                out[b, p, :] = hit[0]
                out[b, p, :len(hit)] = hit
    return out


def bitrev(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def fps_np(xyz, m, bs):
    """FPS with the closed-form tie rule derived in DESIGN.md: among maximal points the winner
    minimises (bitrev(k mod bs), k div bs).  Independent of the oracle's literal block emulation."""
    n = xyz.shape[0]
    bits = int(np.log2(bs))
    k = np.arange(n)
    key = np.array([bitrev(int(i % bs), bits) for i in k], np.int64) * (n // bs + 2) + k // bs
    temp = np.full(n, 1e10, np.float32)
    sel = [0]
    for _ in range(1, m):
        d = xyz - xyz[sel[-1]][None]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        temp = np.minimum(d2, temp)
        cand = np.nonzero(temp == temp.max())[0]
        sel.append(int(cand[np.argmin(key[cand])]))
    return np.array(sel, np.int32)


def clip_area64(pa, pb):
    """float64 Sutherland-Hodgman intersection area of two convex polygons (CCW)."""
    def area(p):
        x, y = p[:, 0], p[:, 1]
        return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))

    def ccw(p):
        x, y = p[:, 0], p[:, 1]
        return p if (np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))) > 0 else p[::-1]
    out = ccw(pa.astype(np.float64))
    clip = ccw(pb.astype(np.float64))
    for i in range(len(clip)):
        a, b = clip[i], clip[(i + 1) % len(clip)]
        inp, out = out, []
        if len(inp) == 0:
            break
        for j in range(len(inp)):
            p, q = inp[j], inp[(j + 1) % len(inp)]
            sp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
            sq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
            if sp >= 0:
                out.append(p)
            if sp * sq < 0:
                t = sp / (sp - sq)
                out.append(p + t * (q - p))
        out = np.array(out)
    return area(out) if len(out) >= 3 else 0.0


def bev_corners64(b):
    """iou3d box [x1,y1,x2,y2,ry]: corners rotated about the centre by the kernel's matrix."""
    cx, cy = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
    pts = np.array([[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]], np.float64)
    c, s = np.cos(np.float64(b[4])), np.sin(np.float64(b[4]))
    dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
    return np.stack([dx * c + dy * s + cx, -dx * s + dy * c + cy], 1)


def centre_corners64(b):
    """rotate_iou box [cx,cy,w,h,angle] (rotate_iou.py:203-228)."""
    c, s = np.cos(np.float64(b[4])), np.sin(np.float64(b[4]))
    px = np.array([-b[2] / 2, -b[2] / 2, b[2] / 2, b[2] / 2], np.float64)
    py = np.array([-b[3] / 2, b[3] / 2, b[3] / 2, -b[3] / 2], np.float64)
    return np.stack([c * px + s * py + b[0], -s * px + c * py + b[1]], 1)


# ---------------------------------------------------------------- tests
def test_opt_n_threads(oracle):
    assert [oracle.opt_n_threads(n) for n in (16384, 4096, 1024, 512, 128, 1000, 100, 3, 1)] == \
        [1024, 1024, 1024, 512, 128, 512, 64, 2, 1]


def test_ball_query_vs_numpy_and_golden(oracle):
    g = load("g_ops_oracle.npz")
    xyz, new = g["bq_xyz"], g["bq_new"]
    for r in (0.1, 0.2, 0.4, 2.0):
        for ns in (16, 32, 64):
            got = oracle.ball_query(r, ns, xyz, new)
            assert np.array_equal(got, g["bq_r%g_ns%d" % (r, ns)])
            if ns == 16 or r == 0.4:
                assert np.array_equal(got, ball_query_np(r, ns, xyz, new))
    assert (oracle.ball_query(0.4, 32, xyz, new)[0, 0] == 0).all()          # empty ball keeps the zero fill
    full = oracle.ball_query(2.0, 16, xyz, new)
    row = full[1, 5].astype(np.int64)                                        # duplicate cloud: k and k+512
    cnt = 1 + int(np.argmax(np.diff(row) <= 0)) if (np.diff(row) <= 0).any() else len(row)
    assert (np.diff(row[:cnt]) > 0).all() and (row[cnt:] == row[0]).all()    # index order, then back-fill
    assert cnt >= 2 and row[1] == row[0] + 512


def test_fps_tie_rule_vs_closed_form_and_golden(oracle):
    g = load("g_ops_oracle.npz")
    for n, m in ((128, 32), (512, 128), (1000, 100), (1024, 256), (2048, 512)):
        for kind in ("lat", "rnd"):
            cloud = g["fps_%s_in_%d" % (kind, n)]
            got = oracle.furthest_point_sample(cloud, m)
            assert np.array_equal(got, g["fps_%s_%d" % (kind, n)])
            assert np.array_equal(got[0], fps_np(cloud[0], m, oracle.opt_n_threads(n)))
    # the tie rule really depends on the block size: lattice, bs 64 vs 1024 must differ somewhere
    cloud = g["fps_lat_in_2048"]
    a = oracle.furthest_point_sample(cloud, 256, block_size=64)
    b = oracle.furthest_point_sample(cloud, 256, block_size=1024)
    assert not np.array_equal(a, b)
    assert np.array_equal(a[0], fps_np(cloud[0], 256, 64))


def test_three_nn_vs_numpy(oracle):
    g = load("g_ops_oracle.npz")
    unk, kn = g["nn_unknown"], g["nn_known"]
    d2, idx = oracle.three_nn(unk, kn)
    assert np.array_equal(idx, g["nn_idx"]) and np.array_equal(d2, g["nn_d2"])
    d = unk[0][:, None, :] - kn[0][None]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.argsort(dd, axis=1, kind="stable")[:, :3]                    # stable: lowest index wins ties
    assert np.array_equal(idx[0], order.astype(np.int32))
    assert np.array_equal(d2[0], np.take_along_axis(dd, order, 1))
    w = np.random.default_rng(0).uniform(0, 1, idx.shape).astype(np.float32)
    f = np.random.default_rng(1).standard_normal((1, 7, kn.shape[1])).astype(np.float32)
    want = (w[0, :, 0] * f[0][:, idx[0, :, 0]] + w[0, :, 1] * f[0][:, idx[0, :, 1]]) + w[0, :, 2] * f[0][:, idx[0, :, 2]]
    assert np.array_equal(oracle.three_interpolate(f, idx, w)[0], want)


def test_group_gather_and_grads(oracle):
    rng = np.random.default_rng(2)
    pts = rng.standard_normal((2, 5, 60)).astype(np.float32)
    idx = rng.integers(0, 60, (2, 9, 4)).astype(np.int32)
    assert np.array_equal(oracle.group_points(pts, idx), np.stack([pts[b][:, idx[b]] for b in range(2)]))
    gi = rng.integers(0, 60, (2, 11)).astype(np.int32)
    assert np.array_equal(oracle.gather_points(pts, gi), np.stack([pts[b][:, gi[b]] for b in range(2)]))
    go = rng.standard_normal((2, 5, 9, 4)).astype(np.float32)
    want = np.zeros((2, 5, 60), np.float64)
    for b in range(2):
        for c in range(5):
            np.add.at(want[b, c], idx[b].ravel(), go[b, c].ravel())
    np.testing.assert_allclose(oracle.group_points_grad(go, idx, 60), want, rtol=1e-5, atol=1e-5)


def test_query_and_group_equals_composition(oracle):
    xyz = scenes(1, 512, seed0=5)
    new = xyz[:, :64].copy()
    feats = np.random.default_rng(3).standard_normal((1, 6, 512)).astype(np.float32)
    out, idx = oracle.query_and_group(0.9, 16, xyz, new, feats)
    assert np.array_equal(idx, oracle.ball_query(0.9, 16, xyz, new))
    gx = oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), idx) - new.transpose(0, 2, 1)[..., None]
    assert np.array_equal(out[:, :3], gx) and np.array_equal(out[:, 3:], oracle.group_points(feats, idx))


def test_nms_and_overlap_vs_independent(oracle):
    g = load("g_ops_oracle.npz")
    bx = g["nms_boxes"]
    assert np.array_equal(oracle.nms(bx, 0.1), g["nms_rot_keep"])
    assert np.array_equal(oracle.nms_normal(bx, 0.5), g["nms_norm_keep"])
    np.testing.assert_array_equal(oracle.boxes_overlap_bev(bx[:64], bx[64:128]), g["overlap"])
    # rotated overlap vs float64 polygon clipping
    ov = oracle.boxes_overlap_bev(bx[:40], bx[40:80])
    for i in range(40):
        for j in range(40):
            assert abs(ov[i, j] - clip_area64(bev_corners64(bx[i]), bev_corners64(bx[40 + j]))) < 1e-4
    # greedy axis-aligned NMS in plain python
    def iou_aa(a, b):
        w = max(min(a[2], b[2]) - max(a[0], b[0]), 0); h = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
        inter = np.float32(w) * np.float32(h)
        sa = (a[2] - a[0]) * (a[3] - a[1]); sb = (b[2] - b[0]) * (b[3] - b[1])
        return inter / max(sa + sb - inter, np.float32(1e-8))
    keep = []
    for i in range(len(bx)):
        if all(iou_aa(bx[k], bx[i]) <= np.float32(0.5) for k in keep):
            keep.append(i)
    assert np.array_equal(oracle.nms_normal(bx, 0.5), np.array(keep))
    assert len(oracle.nms(bx[:0], 0.1)) == 0 and list(oracle.nms_normal(bx[:1], 0.5)) == [0]


def test_rotate_iou_vs_clipper_and_golden(oracle):
    g = load("g_ops_oracle.npz")
    cb = g["riou_boxes"]
    for crit in (-1, 0, 1, 2):
        got = oracle.rotate_iou_eval(cb[:50], cb[50:], crit)
        np.testing.assert_array_equal(got, g["riou_c%d" % crit])
    inter = oracle.rotate_iou_eval(cb[:50], cb[50:], 2)
    iou = oracle.rotate_iou_eval(cb[:50], cb[50:], -1)
    for i in range(50):
        for j in range(30):
            a = clip_area64(centre_corners64(cb[i]), centre_corners64(cb[50 + j]))
            assert abs(inter[i, j] - a) < 1e-4
            u = cb[i, 2] * cb[i, 3] + cb[50 + j, 2] * cb[50 + j, 3] - a
            assert abs(iou[i, j] - a / u) < 1e-5
    assert oracle.rotate_iou_eval(cb[:0], cb[50:], -1).shape == (0, 30)


def test_rotate_iou_oracle_equals_the_references_own_python(oracle):
    """K18 pinned to REFERENCE-EXECUTED output: g9 holds what the reference's own evaluate/rotate_iou.py
    (host function :294-329, kernel :261-291, device functions :16-259) computes when its numba / numba.cuda
    imports are served by the interpreter of tests/golden/numba_shim.py (numba's float32 typing rules
    reproduced: f32 (op) f32 -> f32, f32 (op) literal -> f64, stores round).  256 x 256 pairs incl. identical,
    touching, nested, thin, tiny, huge, axis-aligned and far-apart boxes, all four criteria.
    Tolerance: NONE -- the restatement must reproduce the fixture bit for bit.  (What the fixture cannot see is
    CUDA's ``__nv_cosf/__nv_sinf`` and NVVM's fma contraction: both sides use (float) f64-libm trig and no
    contraction)  Pairs flagged ``undefined`` overran the reference's 8-point
    intersection buffer (rotate_iou.py:234) -- undefined behaviour on CUDA; there the oracle only has to be finite."""
    g = load("g9_rotate_iou_ref.npz")
    a, q, und = g["boxes"], g["query_boxes"], g["undefined"]
    assert a.shape == (256, 5) and q.shape == (256, 5) and und.sum() <= 4
    assert (g["iou_c2"] > 0).sum() > 5000                     # thousands of genuinely overlapping pairs
    for crit in (-1, 0, 1, 2):
        got = oracle.rotate_iou_eval(a, q, crit)
        want = g["iou_c%d" % crit]
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got[~und].view(np.uint32), want[~und].view(np.uint32))
    # the classes the fixture was built to hold (make_golden.g9_boxes)
    iou = g["iou_c-1"]
    d = np.arange(16)
    # IDENTICAL boxes: the reference's algorithm lists every shared corner twice (both point_in_quadrilateral tests
    # pass, rotate_iou.py:183-192) and its fan triangulation over the sorted duplicates returns 0, 1/3 or 1 -- a
    # property of the reference that the fixture records and the restatement must (and does) reproduce.
    assert set(np.round(iou[d, d].astype(np.float64), 3).tolist()) <= {0.0, 0.333, 1.0} and (iou[d, d] < 0.5).any()
    assert np.all(iou[96:112] == 0)                           # far apart
    nested = g["iou_c0"][np.arange(56, 72), np.arange(56, 72)]   # criterion 0 divides by rbox1 = the QUERY box (:287-291)
    assert np.all(np.abs(nested - 1) < 1e-4)                  # nested at another angle: inter / area(query) = 1


def test_rotate_iou_live_reference_run_matches_oracle(oracle):
    """The same pin on a second, independent sample: g9l holds what a live run of the reference's rotate_iou.py under the
    interpreter produced on 70 x 20 fresh random boxes (70 rows: two thread blocks, the second one ragged), criteria -1 and 1
    (tests/golden/make_golden.py g9l); the oracle must reproduce it bit for bit wherever the reference is defined."""
    g = load("g9l_rotate_iou_sample_ref.npz")
    a, q = g["boxes"], g["query_boxes"]
    assert a.shape == (70, 5) and q.shape == (20, 5)
    for crit in (-1, 1):
        ref, und = g["iou_c%d" % crit], g["undefined_c%d" % crit]
        got = oracle.rotate_iou_eval(a, q, crit)
        assert (ref > 0).sum() > 200
        np.testing.assert_array_equal(got[~und].view(np.uint32), ref[~und].view(np.uint32))


def test_roipool_vs_compiled_reference_fixture(oracle):
    """g5 holds outputs of the reference's OWN roipool3d.cpp CPU functions (compiled in the build
    container, oracle/Makefile): the oracle must reproduce them bit for bit."""
    g = load("g5_roipool_ref.npz")
    flag = oracle.pts_in_boxes3d(g["pts"], g["boxes"])
    assert np.array_equal(flag, g["pts_flag"].astype(np.int64))
    pp, pf, pe = oracle.roipool3d_cpu(g["pts"], g["boxes"], g["feat"], 512)
    assert np.array_equal(pe, g["pooled_empty_flag"]) and pe.sum() >= 1
    assert np.array_equal(pp, g["pooled_pts"]) and np.array_equal(pf, g["pooled_features"])
    # batched GPU-semantics variant == CPU variant with xyz and features side by side
    pooled, empty = oracle.roipool3d(g["pts"][None], g["boxes"][None], g["feat"][None], 512)
    assert np.array_equal(empty[0], pe.astype(np.int32))
    assert np.array_equal(pooled[0][..., :3], pp) and np.array_equal(pooled[0][..., 3:], pf)
    counts = g["pts_flag"].sum(1)
    assert counts.max() > 512 and ((counts > 0) & (counts < 512)).any()      # full, partial and empty boxes


def test_trig_contract_vs_glibc_sincosf(oracle):
    """The contract is (float)libm_f64(x).  The reference's HOST code (roipool3d.cpp:88) resolves to
    glibc sincosf, which is within 1 ulp of that but not always equal: measure how often (about 1.3 %,
    stated in DESIGN.md).  A point/box decision can differ only for a point within ~1 ulp of a box
    face; the g5 fixture (reference-compiled outputs) is reproduced exactly."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.sincosf.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    x = np.random.default_rng(0).uniform(-np.pi, np.pi, 20000).astype(np.float32)
    s, c = ctypes.c_float(), ctypes.c_float()
    diff = 0
    for v in x:
        libm.sincosf(float(v), ctypes.byref(s), ctypes.byref(c))
        want_c, want_s = np.float32(np.cos(np.float64(v))), np.float32(np.sin(np.float64(v)))
        diff += (np.float32(c.value) != want_c) + (np.float32(s.value) != want_s)
        assert abs(np.float32(c.value) - want_c) <= np.spacing(np.abs(want_c)) * 1.01
    assert diff / (2 * len(x)) < 0.03
