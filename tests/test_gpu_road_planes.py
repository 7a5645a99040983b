"""Road-plane estimation on the device (csrc/road_planes.hip through road_planes.estimate_planes) against the package's own cpu path
and against KNOWN synthetic planes (tests/planes_tree.py): every integer and flag equal, the plane and rms to 1e-9 (only the moment
sums differ between the paths, and only in order: at most 2^15 f64 terms, the 3 x 3 solve shifted to p0)."""
import importlib
import os

import numpy as np
import pytest
import torch

import planes_tree as T

pytestmark = pytest.mark.gpu

PKG = "3d_adapt_auto_driving_amd"
R = importlib.import_module(PKG + ".road_planes")
quiet = lambda s: None
ITERS = 70                                                   # not a multiple of 64
KW = dict(iters=ITERS, min_inliers=30)
IDS = [3, 17, 5, 8, 2, 40, 41, 7, 9, 1]
INTS = ("candidates", "best_hypothesis", "ransac_inliers", "inliers", "fallback")


def mixed_batch():
    """0 points; 2 candidates; 63, 64, 65 candidates (tile edges); 512; 4097; 20000; every point outside the range; one repeated point"""
    cal = T.calib_dict()
    scenes = [(np.zeros((0, 4), np.float32), cal)]
    for k, (n, outside) in enumerate(((2, 5), (63, 40), (64, 40), (65, 40), (512, 100), (4097, 300), (20000, 1000))):
        scenes.append(T.scene(900 + k, n, *T.seeded_pose(900 + k), outside=outside))
    rng = np.random.default_rng(5)
    far = np.stack([rng.uniform(-20, 20, 300), rng.uniform(-1, 2, 300), rng.uniform(60, 70, 300)], 1)
    scenes.append((T.to_lidar(far), cal))
    scenes.append((T.to_lidar(np.tile([[1.5, 1.6, 12.0]], (100, 1))), cal))
    return scenes


@pytest.fixture(scope="module")
def batch():
    scenes = mixed_batch()
    cpu = R.estimate_planes(scenes, device="cpu", ids=IDS, details=True, **KW)
    dev = R.estimate_planes(scenes, device="cuda", ids=IDS, details=True, **KW)
    return scenes, cpu, dev


def same_scene(a_plane, a_info, b_plane, b_info):
    return a_plane.tobytes() == b_plane.tobytes() and all(a_info[k] == b_info[k] for k in INTS) and \
        np.float64(a_info["rms"]).tobytes() == np.float64(b_info["rms"]).tobytes()


def test_device_equals_the_cpu_path_on_one_mixed_batch(batch):
    scenes, (cp, ci), (dp, di) = batch
    assert [i["candidates"] for i in ci] == [0, 2, 63, 64, 65, 512, 4097, 20000, 0, 100]
    assert [i["fallback"] for i in ci] == [R.FALLBACK_REASONS[k] for k in (1, 1, 0, 0, 0, 0, 0, 0, 1, 2)]
    for s, (c, d) in enumerate(zip(ci, di)):
        assert d["candidates"] == c["candidates"], s
        assert d["candidate_points"].dtype == np.float32 and d["candidate_points"].tobytes() == c["candidate_points"].tobytes(), s
        assert np.array_equal(d["accepted"], c["accepted"]) and np.array_equal(d["scores"], c["scores"]), s
        assert all(d[k] == c[k] for k in INTS), (s, d, c)
        print("scene %d: plane difference %.3e, rms difference %.3e" % (s, np.abs(dp[s] - cp[s]).max(), abs(d["rms"] - c["rms"])))
        assert np.abs(dp[s] - cp[s]).max() <= 1e-9 and abs(d["rms"] - c["rms"]) <= 1e-9, s
        assert dp[s][1] < 0 and dp[s][3] > 0 and abs(np.linalg.norm(dp[s][0:3]) - 1.0) < 1e-12


def test_single_scene_calls_and_the_reversed_batch_give_the_same_bytes(batch):
    scenes, _, (dp, di) = batch
    for s in range(len(scenes)):
        p, i = R.estimate_planes([scenes[s]], device="cuda", ids=[IDS[s]], **KW)
        assert same_scene(p[0], i[0], dp[s], di[s]), s
    p, i = R.estimate_planes(scenes[::-1], device="cuda", ids=IDS[::-1], **KW)
    for s in range(len(scenes)):
        assert same_scene(p[len(scenes) - 1 - s], i[len(scenes) - 1 - s], dp[s], di[s]), s


def test_two_calls_give_identical_bytes(batch):
    scenes, _, (dp, di) = batch
    p, i = R.estimate_planes(scenes, device="cuda", ids=IDS, details=True, **KW)
    assert p.tobytes() == dp.tobytes()
    for a, b in zip(i, di):
        assert same_scene(p[0], a, p[0], b) and np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["accepted"], b["accepted"])


def test_known_plane_on_the_device():
    picks = (0, 1, 2, 13, 26, 39)                            # six of the cpu test's scenes, every size among them
    scenes, truths = zip(*[T.recovery_scene(k) for k in picks])
    planes, infos = R.estimate_planes(scenes, device="cuda", iters=256, ids=list(picks))
    for k, p, t, info in zip(picks, planes, truths, infos):
        angle, height = T.plane_error(p, t)
        print("scene %d: %.6f deg, %.6f m" % (k, angle, height))
        assert info["fallback"] is None and angle < 0.1 and height < 0.02


def test_the_tool_writes_the_cpu_path_s_files(tmp_path):
    root = str(tmp_path / "tree")
    ids = T.write_tree(root)
    a, b = str(tmp_path / "cuda"), str(tmp_path / "cpu")
    on_dev = R.generate_planes(root, save_dir=a, device="cuda", iters=128, batch=4, log=quiet)
    on_cpu = R.generate_planes(root, save_dir=b, device="cpu", iters=128, batch=4, log=quiet)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == sorted(["%06d.txt" % i for i in ids] + [R.LOG_NAME])
    exits = 0
    for (i, pd, _), (_, pc, _) in zip(on_dev, on_cpu):
        ta, tb = (open(os.path.join(d, "%06d.txt" % i)).read() for d in (a, b))
        if ta == tb:
            continue
        la, lb = ta.splitlines(), tb.splitlines()
        print("scene %06d:\n  cuda %s\n  cpu  %s\n  cuda %r\n  cpu  %r" % (i, la[3], lb[3], pd.tolist(), pc.tolist()))
        assert la[0:3] == lb[0:3] and len(la) == len(lb) == 4 and np.abs(pd - pc).max() <= 1e-9
        for va, vb in zip(la[3].split(), lb[3].split()):
            if va != vb:                                     # the same text but for the last printed digit of the mantissa
                exits += 1
                (ma, ea), (mb, eb) = va.split("e"), vb.split("e")
                assert ea == eb and ma[:-1] == mb[:-1], (va, vb)
    assert exits <= 1


def raises_on_sync(fn):
    """Does ``fn`` perform a blocking device operation?  (torch raises on one under set_sync_debug_mode("error"))"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn()
    except RuntimeError as e:
        assert "synchroniz" in str(e).lower(), e
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_one_blocking_host_read_per_call(batch):
    """The call is upload + launches (road_planes._launch_device: nothing in it blocks) and ONE read of ``out`` behind them."""
    scenes, _, (dp, _) = batch
    probe = torch.ones(1, device="cuda")
    if not raises_on_sync(probe.item):
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is not live on this build: a plain .item() does not raise under it")
    p = R._Params(ITERS, 0.2, 15.0, (-20, 20), (0, 50), KW["min_inliers"], 1.65)
    clouds, calibs = [np.ascontiguousarray(pts) for pts, _ in scenes], [R.as_calib(c) for _, c in scenes]
    draws = [R.draws_of(0, i, ITERS) for i in IDS]
    got = []
    assert not raises_on_sync(lambda: got.append(R._launch_device(clouds, calibs, draws, p, "cuda")))
    assert got[0][1]["out"].cpu().numpy()[:, 0:4].tobytes() == dp.tobytes()       # ... and the one read gives the call's planes
    assert raises_on_sync(lambda: R.estimate_planes(scenes, device="cuda", ids=IDS, **KW))   # the whole call does block: on that read
