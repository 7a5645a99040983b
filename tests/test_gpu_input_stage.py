"""Device input stage (csrc/input_stage.hip) vs the host numpy stage (kitti_io: Calibration, valid_flag; synth.subsample_rpn
restating kitti_rcnn_dataset.py:288-324).  The subset is random on both sides, so against the host sampler the device's is checked
through its invariants and its distribution; the transform + filter are compared point by point.  Against its own rule the
device sampler is determined row for row: tests/input_stage_ref.py is the definition, and the second half of this file compares
choice, stats and out with it as bits on every branch."""
import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def stage(far=4000, seed=1024):
    C, K = pkg("config"), pkg("kitti_io")
    cfg = C.default_eval_cfg()
    return cfg, K.DeviceInputStage(cfg, DEV, npoints_faraway=far, seed=seed), pkg("synth").SyntheticCalib()


def run(st, raws, ids, calib, **kw):
    shapes = [calib.image_shape] * len(raws)
    out, stats, choice = st(raws, [calib] * len(raws), shapes, ids, return_choice=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), choice.cpu().numpy()


def test_sampler_invariants_large_cloud():
    """More valid points than npoints: every far point up to the cap, the rest near, no duplicates, outputs are bitwise
    copies of the chosen raw points, deterministic in the seed, different for another scene id."""
    cfg, st, calib = stage()
    rng = np.random.default_rng(0)
    N = cfg.RPN.NUM_POINTS
    clouds = []
    for n_far in (1500, 9000, 0):
        near = rng.uniform([-40, -1, 0], [40, 3, 39.99], (50000, 3))
        far = rng.uniform([-40, -1, 40.0], [40, 3, 70.4], (n_far, 3))
        pts = np.concatenate([near, far]).astype(np.float32)
        clouds.append(pts[rng.permutation(len(pts))])
    out, stats, choice = run(st, clouds, [5, 6, 7], calib, lidar_frame=False, image_filter=False)
    for b, pts in enumerate(clouds):
        ch = choice[b]
        assert stats[b, 0] == len(pts) and stats[b, 2] == int((pts[:, 2] >= 40.0).sum())
        assert ch.min() >= 0 and ch.max() < len(pts) and len(np.unique(ch)) == N          # without replacement
        assert np.array_equal(out[b], pts[ch])
        n_far = int(stats[b, 2])
        assert int((pts[ch, 2] >= 40.0).sum()) == min(n_far, 4000)
    same_bits((out, stats, choice), want_of(st, cfg, clouds, [5, 6, 7]))                   # every row is the definition's
    out2, _, choice2 = run(st, clouds, [5, 6, 7], calib, lidar_frame=False, image_filter=False)
    assert np.array_equal(choice, choice2) and np.array_equal(out, out2)
    _, _, choice3 = run(st, clouds[:1], [99], calib, lidar_frame=False, image_filter=False)
    assert not np.array_equal(choice3[0], choice[0])
    assert len(np.intersect1d(choice3[0], choice[0])) < 0.6 * N                            # ~31 % overlap expected


def test_sampler_small_clouds_and_empty():
    """Fewer valid points than npoints: every point present; the extra copies are distinct points when they fit
    (each index at most twice), drawn with replacement otherwise; an all-invalid scene gives zeros."""
    cfg, st, calib = stage()
    rng = np.random.default_rng(1)
    N = cfg.RPN.NUM_POINTS
    a = rng.uniform([-40, -1, 0], [40, 3, 70], (12000, 3)).astype(np.float32)             # extra 4384 <= 12000
    b = rng.uniform([-40, -1, 0], [40, 3, 70], (100, 3)).astype(np.float32)               # extra > n: with replacement
    c = np.full((500, 3), 1000.0, np.float32)                                             # outside PC_AREA_SCOPE
    d = rng.uniform([-40, -1, 0], [40, 3, 70], (N, 3)).astype(np.float32)                 # exactly npoints
    out, stats, choice = run(st, [a, b, c, d], [1, 2, 3, 4], calib, lidar_frame=False, image_filter=False)
    cnt = np.bincount(choice[0], minlength=len(a))
    assert cnt.min() == 1 and cnt.max() == 2 and int((cnt == 2).sum()) == N - len(a)
    assert np.array_equal(out[0], a[choice[0]])
    cnt = np.bincount(choice[1], minlength=len(b))
    assert cnt.min() >= 1 and cnt.sum() == N and cnt.max() < 3 * N // len(b)
    assert stats[2, 0] == 0 and (choice[2] == -1).all() and (out[2] == 0).all()
    assert np.array_equal(np.sort(choice[3]), np.arange(N))                               # a permutation
    assert not np.array_equal(choice[3], np.arange(N))                                    # ... that is shuffled
    same_bits((out, stats, choice), want_of(st, cfg, [a, b, c, d], [1, 2, 3, 4]))         # and every row is the definition's


def test_sampler_distribution():
    """Selection frequency per point over many seeds is binomial (uniform subset), and the output position of a point
    is uncorrelated with its index (uniform shuffle)."""
    cfg, st, calib = stage()
    rng = np.random.default_rng(2)
    N = cfg.RPN.NUM_POINTS
    n = 40000
    pts = rng.uniform([-40, -1, 0], [40, 3, 39.9], (n, 3)).astype(np.float32)
    seeds = 48
    freq = np.zeros(n)
    corr = []
    for s0 in range(0, seeds, 8):
        _, _, choice = run(st, [pts] * 8, list(range(s0, s0 + 8)), calib, lidar_frame=False, image_filter=False)
        for ch in choice:
            freq[ch] += 1
            corr.append(np.corrcoef(ch.astype(np.float64), np.arange(N))[0, 1])
    p = N / n
    assert abs(freq.mean() - seeds * p) < 1e-9
    var = freq.var()
    assert 0.85 * seeds * p * (1 - p) < var < 1.15 * seeds * p * (1 - p), var           # binomial variance
    assert max(abs(c) for c in corr) < 0.05
    lo, hi = freq[: n // 2].mean(), freq[n // 2:].mean()
    assert abs(lo - hi) < 0.15                                                              # no index bias


def test_transform_and_filter_match_host_stage():
    """Lidar-frame input with a KITTI-like calibration: the points the device keeps are the points the numpy stage
    keeps (borderline roundings aside), and their rectified coordinates agree."""
    K = pkg("kitti_io")
    cfg, st, _ = stage()
    rng = np.random.default_rng(3)
    calib = K.Calibration({
        "P2": [721.5377, 0, 609.5593, 44.85728, 0, 721.5377, 172.854, 0.2163791, 0, 0, 1, 0.002745884],
        "R0": [0.9999239, 0.00983776, -0.007445048, -0.009869795, 0.9999421, -0.004278459, 0.007402527, 0.004351614, 0.9999631],
        "Tr_velo2cam": [0.007533745, -0.9999714, -0.000616602, -0.004069766, 0.01480249, 0.0007280733, -0.9998902, -0.07631618,
                        0.9998621, 0.007523790, 0.01480755, -0.2717806]})
    shape = (375, 1242, 3)
    n = 110000
    lidar = np.concatenate([rng.uniform([-10, -60, -3], [90, 60, 2], (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    out, stats, choice = st([lidar], [calib], [shape], [42], lidar_frame=True, image_filter=True, return_choice=True)
    torch.cuda.synchronize()
    out, stats, choice = out.cpu().numpy()[0], stats.cpu().numpy()[0], choice.cpu().numpy()[0]
    rect = calib.lidar_to_rect(lidar[:, :3])
    img, depth = calib.rect_to_img(rect)
    flag = K.valid_flag(rect, img, depth, shape, cfg.PC_AREA_SCOPE if cfg.PC_REDUCE_BY_RANGE else None)
    n_host = int(flag.sum())
    # round 4: the device reproduces numpy's float32 arithmetic (fma chains), so the two stages agree exactly wherever this
    # host's BLAS computes np.dot the way the reference fixture's host did (g11 pins the device to the reference-made data;
    # here a handful of borderline roundings are tolerated in case another CPU's sgemm kernel accumulates differently)
    assert abs(int(stats[0]) - n_host) <= 3, (stats, n_host)
    assert flag[choice].mean() > 0.9995
    assert np.abs(out - rect[choice]).max() < 2e-5
    print("device vs host numpy: valid %d / %d, max |d rect| %.3g" % (int(stats[0]), n_host, float(np.abs(out - rect[choice]).max())))
    far_host = int((flag & (rect[:, 2] >= 40.0)).sum())
    assert abs(int(stats[2]) - far_host) <= 3
    N = cfg.RPN.NUM_POINTS
    assert n_host > N
    far_keep = min(int(stats[2]), 4000)
    n_near = int(stats[1])
    assert int((rect[choice, 2] >= 40.0).sum()) == far_keep
    if n_near >= N - far_keep:
        assert len(np.unique(choice)) == N
    else:                                   # too few near points: every near point once + copies, every kept far point once
        cnt = np.bincount(choice, minlength=n)
        near_idx = np.where(flag & (rect[:, 2] < 40.0))[0]
        assert (cnt[near_idx] >= 1).mean() > 0.999 and len(np.unique(choice)) >= n_near + far_keep - 3


def test_device_filter_equals_reference_executed_flags(tmp_path):
    """g11: the reference's OWN lidar_to_rect / rect_to_img / get_valid_flag (calibration.py:51-71, kitti_rcnn_dataset.py:201-222)
    were run on the five scenes of the fake KITTI tree (regenerated here from the seed).  The device stage must produce the
    SAME flag for every raw point and the same rectified coordinates bit for bit (float32 np.dot = fma chains over the inner
    index, reproduced in csrc/input_stage.hip), and its sampler must take each of the reference sampler's branches with the
    reference's counts (all far points up to the cap / every point once + copies / copies with replacement)."""
    import os
    import helpers
    K = pkg("kitti_io")
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g11_input_writer_ref.npz"))
    cfg, st, _ = stage()
    ids = helpers.write_fake_kitti_tree(str(tmp_path), int(g["seed"]), with_images=False)
    src = K.KittiSource(str(tmp_path), cfg, split="val")
    raws, calibs, shapes = [], [], []
    for sid in ids:
        lidar, calib, _ = src.load_raw(sid)
        assert abs(float(lidar.astype(np.float64).sum()) - float(g["lidar_sum_%d" % sid])) < 1e-9, "the regenerated tree differs"
        raws.append(lidar); calibs.append(calib); shapes.append(tuple(g["shape_%d" % sid]) + (3,))
    cls, rect = K.device_valid_flags(cfg, DEV, raws, calibs, shapes)
    cls, rect = cls.cpu().numpy(), rect.cpu().numpy()
    out, stats, choice = st(raws, calibs, shapes, ids, lidar_frame=True, image_filter=True, return_choice=True)
    torch.cuda.synchronize()
    out, stats, choice = out.cpu().numpy(), stats.cpu().numpy(), choice.cpu().numpy()
    N = cfg.RPN.NUM_POINTS
    for b, sid in enumerate(ids):
        n = len(raws[b])
        want = np.unpackbits(g["valid_%d" % sid])[:n].astype(bool)
        assert np.array_equal(cls[b, :n] > 0, want), (sid, int(((cls[b, :n] > 0) != want).sum()))
        assert (cls[b, n:] == 0).all()
        assert np.array_equal(rect[b, :n][::97], g["rect_sub_%d" % sid]), sid             # the reference's rectified coordinates
        z = rect[b, :n, 2]
        assert np.array_equal(cls[b, :n] == 2, want & (z >= 40.0))
        nv, nf = int(want.sum()), int((want & (z >= 40.0)).sum())
        assert stats[b].tolist() == [nv, nv - nf, nf]
        ch = choice[b]
        assert want[ch].all() and np.array_equal(out[b], rect[b, ch])
        assert np.array_equal(ch, ref().sample_choice(cls[b, :n], N, 4000, st.seed + sid))   # the definition's rows, lidar frame + image filter
        # the reference's own choice on this scene and the device's: the same branch, the same class counts
        ref_choice = np.nonzero(want)[0][g["choice_%d" % sid]]
        if nv > N:                                           # far points: all of them up to the cap, on both sides
            assert int((z[ch] >= 40.0).sum()) == int((z[ref_choice] >= 40.0).sum()) == min(nf, 4000)
            if nv - nf >= N - min(nf, 4000):                 # enough near points: no copies
                assert len(np.unique(ch)) == len(np.unique(ref_choice)) == N
        if nv <= N:
            assert len(np.unique(ch)) == nv == len(np.unique(ref_choice))                 # every valid point at least once


# ---- the sampler against its definition (tests/input_stage_ref.py): choice, stats and out == rect[choice], bit for bit
def small_stage(npoints, far, seed=1024):
    C, K = pkg("config"), pkg("kitti_io")
    cfg = C.default_eval_cfg()
    C.merge_into({"RPN": {"NUM_POINTS": npoints}}, cfg)
    return cfg, K.DeviceInputStage(cfg, DEV, npoints_faraway=far, seed=seed), pkg("synth").SyntheticCalib()


def run_packed(st, clouds, ids, calib):
    """The clouds as one ragged block whose rows beyond a cloud's length are NaN (DeviceInputStage.from_packed)."""
    n_max, stride = max(1, max(len(c) for c in clouds)), clouds[0].shape[1]
    host = torch.full((len(clouds), n_max, stride), float("nan"), dtype=torch.float32)
    for i, c in enumerate(clouds):
        host[i, :len(c)] = torch.from_numpy(c)
    shapes = [calib.image_shape] * len(clouds)
    out, stats, choice = st.from_packed(host.pin_memory(), [len(c) for c in clouds], [calib] * len(clouds), shapes, ids,
                                        lidar_frame=False, image_filter=False, return_choice=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), choice.cpu().numpy()


def want_of(st, cfg, clouds, ids, classes=None):
    """The definition's (out, stats, choice) of every scene, stacked; ``classes``: the class of every point where the test made it"""
    R = ref()
    rows = []
    for b, (c, i) in enumerate(zip(clouds, ids)):
        cls = R.classify(c[:, :3], cfg.PC_AREA_SCOPE, st.far_depth) if classes is None else classes[b]
        rows.append(R.expected(c, cls, cfg.RPN.NUM_POINTS, st.npoints_faraway, st.seed + i))
    return tuple(np.stack(x, 0) for x in zip(*rows))


def same_bits(got, want):
    out, stats, choice = got
    w_out, w_stats, w_choice = want
    assert np.array_equal(choice, w_choice), [int((a != b).sum()) for a, b in zip(choice, w_choice)]
    assert np.array_equal(stats, w_stats), (stats.tolist(), w_stats.tolist())
    assert out.dtype == w_out.dtype == np.float32 and np.array_equal(out.view(np.uint32), w_out.view(np.uint32))


def ref():
    import input_stage_ref
    return input_stage_ref


def test_sampler_equals_definition_on_every_branch():
    """Every branch of the sampler at npoints = 256, cap 64 (tests/input_stage_ref.py BRANCH_CASES): one ragged batch with NaN
    behind every cloud, each cloud alone, a second call and a side stream all give the definition's bytes."""
    R = ref()
    cfg, st, calib = small_stage(256, 64)
    rng = np.random.default_rng(21)
    clouds = [R.make_cloud(*tri, rng) for tri, _ in R.BRANCH_CASES]
    ids = list(range(30, 30 + len(clouds)))
    traces = []
    for c, i in zip(clouds, ids):
        traces.append(set())
        R.sample_choice(R.classify(c, R.SCOPE, R.FAR_DEPTH), 256, 64, st.seed + i, traces[-1])
    assert all(want <= t for (_, want), t in zip(R.BRANCH_CASES, traces)), traces
    want = want_of(st, cfg, clouds, ids)
    batch = run_packed(st, clouds, ids, calib)
    same_bits(batch, want)
    same_bits(run_packed(st, clouds, ids, calib), want)                                        # the same call a second time
    same_bits(run(st, clouds, ids, calib, lidar_frame=False, image_filter=False), want)       # the staged form
    for b, (c, i) in enumerate(zip(clouds, ids)):
        same_bits(run(st, [c], [i], calib, lidar_frame=False, image_filter=False), tuple(x[b:b + 1] for x in want))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = run_packed(st, clouds, ids, calib)
    same_bits(again, want)


def test_sampler_equals_definition_other_shapes():
    """npoints that is no power of two (sort pad 1024) with far_keep = npoints, npoints = 1, clouds around the workgroup's stride
    of 1024 on the large, the distinct-extras and the with-replacement branch, and 70 000 points."""
    R = ref()
    rng = np.random.default_rng(22)
    cfg, st, calib = small_stage(1000, 4000)
    clouds = [R.make_cloud(500, 1500, 20, rng), R.make_cloud(300, 100, 7, rng), R.make_cloud(999, 0, 0, rng)]
    same_bits(run_packed(st, clouds, [1, 2, 3], calib), want_of(st, cfg, clouds, [1, 2, 3]))
    cfg, st, calib = small_stage(1, 4000)
    clouds = [R.make_cloud(5, 3, 2, rng), R.make_cloud(0, 2, 0, rng), R.make_cloud(1, 0, 0, rng), R.make_cloud(0, 0, 3, rng)]
    same_bits(run_packed(st, clouds, [4, 5, 6, 7], calib), want_of(st, cfg, clouds, [4, 5, 6, 7]))
    cfg, st, calib = small_stage(256, 64)
    clouds = []
    for n in (1023, 1024, 1025):
        clouds += [R.make_cloud(700, 300, n - 1000, rng), R.make_cloud(150, 50, n - 200, rng), R.make_cloud(90, 30, n - 120, rng),
                   R.make_cloud(60, 300, n - 360, rng)]
    clouds.append(R.make_cloud(60000, 9000, 1000, rng))
    clouds.append(R.make_cloud(100, 400, 69500, rng))                 # the ordered compaction over 69 rounds
    ids = list(range(8, 8 + len(clouds)))
    same_bits(run_packed(st, clouds, ids, calib), want_of(st, cfg, clouds, ids))


def test_radix_select_with_every_key_in_one_bin():
    """70 000 points of which exactly those are valid whose selection key has top byte 0x00 (268 of them with seed 1031), in a
    second scene 0xff (251): with npoints = 200 the first pass of the radix select finds every candidate in its first / last bin.
    Then the same with the valid points split into two classes (cap 64)."""
    R = ref()
    cfg, st, calib = small_stage(200, 4000, seed=1024)
    n, sid = 70000, 7
    top = (R.selection_keys(n, st.seed + sid) >> np.uint64(24)).astype(np.int64)
    assert int((top == 0).sum()) == 268 and int((top == 255).sum()) == 251
    rng = np.random.default_rng(23)
    clouds, classes = [], []
    for byte in (0, 255):
        for split in (False, True):
            pts = rng.uniform([-40, -1, 0], [40, 3, 39.9], (n, 3)).astype(np.float32)
            valid = top == byte
            pts[~valid, 1] = np.float32(3.5)                          # outside the scope
            if split:
                far = valid & (rng.random(n) < 0.5)
                pts[far, 2] = pts[far, 2] * np.float32(0.7) + np.float32(40.1)      # 40.1 <= z < 68.1
            clouds.append(pts)
            classes.append(R.classify(pts, R.SCOPE, R.FAR_DEPTH))
            assert np.array_equal(classes[-1] > 0, valid)
    same_bits(run_packed(st, clouds[0::2], [sid, sid], calib), want_of(st, cfg, clouds[0::2], [sid, sid], classes[0::2]))
    cfg, st, calib = small_stage(200, 64, seed=1024)
    same_bits(run_packed(st, clouds[1::2], [sid, sid], calib), want_of(st, cfg, clouds[1::2], [sid, sid], classes[1::2]))


def test_seed_words_and_the_constant_shuffle_word():
    """A seed with a non-zero high word, one with bit 31 set and the default; two scene ids take different subsets but put the raw
    indices they share in the same relative order (the shuffle word depends on the seed's high half alone)."""
    R = ref()
    rng = np.random.default_rng(24)
    clouds = [R.make_cloud(1000, 200, 50, rng), R.make_cloud(100, 500, 9, rng), R.make_cloud(255, 0, 3, rng), R.make_cloud(100, 27, 3, rng)]
    got = {}
    for seed in ((1 << 33) + 5, (1 << 31) + 9, 1024):
        cfg, st, calib = small_stage(256, 64, seed=seed)
        for ids in ([5, 5, 5, 5], [6, 6, 6, 6]):
            got[seed, ids[0]] = run_packed(st, clouds, ids, calib)
            same_bits(got[seed, ids[0]], want_of(st, cfg, clouds, ids))
    a, b = got[1024, 5][2][0], got[1024, 6][2][0]
    shared = np.intersect1d(a, b)
    assert not np.array_equal(np.sort(a), np.sort(b)) and len(shared) > 10
    assert np.array_equal(a[np.isin(a, shared)], b[np.isin(b, shared)])
    c = got[(1 << 33) + 5, 5][2][0]                                     # another high word: another order
    shared = np.intersect1d(a, c)
    assert len(shared) > 10 and not np.array_equal(a[np.isin(a, shared)], c[np.isin(c, shared)])


def test_stride_three_and_four_inputs():
    R = ref()
    rng = np.random.default_rng(25)
    cfg, st, calib = small_stage(256, 64)
    clouds3 = [R.make_cloud(1000, 200, 50, rng), R.make_cloud(100, 500, 9, rng), R.make_cloud(100, 27, 3, rng), R.make_cloud(0, 0, 4, rng)]
    clouds4 = [np.concatenate([c, rng.uniform(0, 1, (len(c), 1)).astype(np.float32)], 1) for c in clouds3]
    want = want_of(st, cfg, clouds3, [1, 2, 3, 4])
    same_bits(run_packed(st, clouds3, [1, 2, 3, 4], calib), want)
    same_bits(run_packed(st, clouds4, [1, 2, 3, 4], calib), want)
    same_bits(run(st, clouds4, [1, 2, 3, 4], calib, lidar_frame=False, image_filter=False), want)


def test_nothing_taken_is_an_empty_scene():
    """npoints_faraway = 0 and more than npoints valid points, all far: no far point may be kept and there is no near one.  The
    kernel leaves through the empty-scene exit (zeros, -1, stats as counted); its neighbours in the batch are untouched."""
    R = ref()
    rng = np.random.default_rng(26)
    cfg, st, calib = small_stage(256, 0)
    clouds = [R.make_cloud(300, 400, 5, rng), R.make_cloud(0, 400, 5, rng), R.make_cloud(0, 200, 5, rng), R.make_cloud(1, 400, 5, rng)]
    got = run_packed(st, clouds, [1, 2, 3, 4], calib)
    same_bits(got, want_of(st, cfg, clouds, [1, 2, 3, 4]))
    out, stats, choice = got
    assert stats[1].tolist() == [400, 0, 400] and (choice[1] == -1).all() and not out[1].view(np.uint32).any()
    assert (choice[[0, 2, 3]] >= 0).all()
    assert (clouds[3][choice[3], 2] < 40.0).all()                        # one near point, 256 times


def test_scope_bounds_are_decided_as_on_the_host():
    """Each bound of PC_AREA_SCOPE and far_depth, the f32 below and the f32 above it, on every axis: the device class equals
    kitti_io.valid_flag on the same array (f32 coordinates against the f64 scope, in double: f32(70.4) is outside) and near / far
    equals z < 40 -- through prcnn_valid_flags and through the stage."""
    R, K = ref(), pkg("kitti_io")
    f = np.float32
    rows = []
    for axis, bounds in ((0, (-40, 40)), (1, (-1, 3)), (2, (0, 40, 70.4))):
        for v in bounds:
            for w in (f(v), np.nextafter(f(v), f(-1000)), np.nextafter(f(v), f(1000))):
                for z_other in (10.0, 50.0):
                    p = [f(1.5), f(1.0), f(z_other)]
                    p[axis] = w
                    rows.append(p)
    pts = np.array(rows, dtype=np.float32)
    cfg, st, calib = small_stage(64, 16)
    flag = K.valid_flag(pts, np.zeros((len(pts), 2), f), np.zeros(len(pts), f), (375, 1242, 3), cfg.PC_AREA_SCOPE)
    z70 = pts[:, 2] == f(70.4)
    assert z70.sum() == 2 and not flag[z70].any() and flag[pts[:, 2] == np.nextafter(f(70.4), f(0))].all()
    want_cls = np.where(flag, np.where(pts[:, 2] < f(40.0), 1, 2), 0)
    assert np.array_equal(R.classify(pts, cfg.PC_AREA_SCOPE, 40.0), want_cls)
    cls, rect = K.device_valid_flags(cfg, DEV, [pts], [calib], [calib.image_shape], lidar_frame=False, image_filter=False)
    assert np.array_equal(cls.cpu().numpy()[0], want_cls), np.nonzero(cls.cpu().numpy()[0] != want_cls)[0]
    assert np.array_equal(rect.cpu().numpy()[0].view(np.uint32), pts.view(np.uint32))
    got = run_packed(st, [pts], [3], calib)
    same_bits(got, want_of(st, cfg, [pts], [3], [want_cls]))
    assert got[1][0].tolist() == [int(flag.sum()), int((want_cls == 1).sum()), int((want_cls == 2).sum())]


def test_production_shape_equals_definition():
    """npoints = 16384, cap 4000: 40 000 valid points (both classes by threshold) and 3 000 (copies with replacement)."""
    R = ref()
    rng = np.random.default_rng(27)
    cfg, st, calib = stage()
    assert cfg.RPN.NUM_POINTS == 16384
    clouds = [R.make_cloud(33000, 7000, 2000, rng), R.make_cloud(2000, 1000, 500, rng)]
    same_bits(run_packed(st, clouds, [11, 12], calib), want_of(st, cfg, clouds, [11, 12]))


def test_eval_scenes_with_device_input_stage():
    """The harness with --device_input: loader processes only read raw clouds, the device does the rest; detections
    come out for every scene (dense 60 k-point synthetic clouds through the sampler)."""
    E, K = pkg("eval_rcnn"), pkg("kitti_io")
    from test_host_logic import tiny_model
    model, cfg, g = tiny_model(DEV)
    src = K.SyntheticSource(cfg, 6, raw_points=60000)
    table, counts = E.eval_scenes(model, cfg, DEV, src, src.ids, batch_size=4, workers=0, device_input=True)
    assert table.shape[0] == 6 and int(counts.min()) >= 0 and torch.isfinite(table).all()
    table2, counts2 = E.eval_scenes(model, cfg, DEV, src, src.ids, batch_size=4, workers=2, device_input=True)
    assert torch.equal(table, table2) and torch.equal(counts, counts2)                    # deterministic in the scene id
