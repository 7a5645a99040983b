"""Beam resampling (3d_adapt_auto_driving_amd/beam_resample.py), host side: the numpy definition against sweeps with a KNOWN ring per
point (tests/beam_tree.py), its edge cases on hand-made points and histograms, and the tool on a six-scene tree.  No fixture comes from
the reference project: it has no counterpart."""
import importlib
import os

import numpy as np
import pytest

import beam_tree as T

PKG = "3d_adapt_auto_driving_amd"
B = importlib.import_module(PKG + ".beam_resample")
quiet = lambda s: None
EDGE_FOV = dict(fov=(-24.0, 8.0), bins=64)                   # edge 48 is 0 degrees: E[48] == 0.0 exactly


def rows(xyz):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32).reshape(-1, 1)], 1)


def label(points, beams, **kw):
    ids, info = B.label_beams([points], beams, device="cpu", **kw)
    return ids[0], info[0]


# ---- ring recovery: a condition on the definition, no tolerance
@pytest.mark.parametrize("beams, azimuths", [(64, 300), (8, 200)])
def test_wall_ring_every_point_gets_its_ring(beams, azimuths):
    pts, rings = T.wall_ring(1, beams, azimuths)
    assert len(pts) == beams * azimuths and set(rings.tolist()) == set(range(beams))
    ids, info = label(pts, beams)
    assert ids.dtype == np.int32 and np.array_equal(ids, rings)
    assert info["clusters"] == beams and info["unassigned"] == 0 and not info["hit_cap"] and (info["counts"] == azimuths).all()
    assert (np.diff(info["centres"]) > 0).all()


def test_open_sky_keeps_the_pattern_around_missing_beams():
    pts, rings = T.open_sky(2, 16, 100, dead=(3, 8))
    present = np.unique(rings)
    assert present[0] == 0 and present[-1] < 15 and 3 not in present and 8 not in present      # the upper beams and the dead ones return nothing
    span = int(present[-1] - present[0] + 1)
    ids, info = label(pts, span)
    assert np.array_equal(ids, rings - present[0])           # the index, not the rank among the non-empty clusters
    assert np.flatnonzero(info["counts"] == 0).tolist() == [3, 8] and info["clusters"] == span - 2
    kept, report = B.resample_scenes([pts], span, stride=2, device="cpu")
    assert kept[0].tobytes() == pts[(rings - present[0]) % 2 == 0].tobytes() and report[0]["kept"] == len(kept[0])


# ---- edge cases
def test_a_point_on_an_edge_lands_in_that_bin():
    E = B.edge_table(**EDGE_FOV)
    assert E[48] == 0.0 and len(E) == 65
    ids, info = label(rows([[5, 0, 0], [0, -3, -0.0], [5, 0, -1e-30], [5, 0, 1e-30]]), 1, **EDGE_FOV)
    assert info["bins"].tolist() == [48, 48, 47, 48]
    pts, table = rows([[1, 0, 0]]), np.arange(-8.0, 57.0) / 8.0
    for i in (0, 1, 17, 63):                                 # t == E[i] through a hand-made table of exact f32 values
        pts[0, 2] = np.float32(table[i])
        assert label(pts, 1, edges=table)[1]["bins"].tolist() == [i]


def test_unassigned_points():
    E = B.edge_table(**EDGE_FOV)
    below = np.float32(np.tan(np.radians(-24.5)))
    assert float(below) < E[0]
    pts = rows([[0, 0, 1], [0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [1, 1, -np.inf], [1, 0, below], [1, 0, 1.0], [2, 0, 0.1]])
    pts[6, 2] = np.float32(np.nextafter(np.float32(E[64]), np.float32(1)))       # t at or above the last edge
    ids, info = label(pts, 2, **EDGE_FOV)
    assert ids.tolist() == [-1, -1, -1, -1, -1, -1, -1, 0] and info["bins"][:7].tolist() == [-1] * 7
    assert info["unassigned"] == 7 and info["points"] == 8 and info["clusters"] == 1
    pts[6, 2] = np.float32(E[64])                            # exactly the last edge where f32 holds it, else the value above or below it
    assert (label(pts, 2, **EDGE_FOV)[0][6] == -1) == (float(np.float32(E[64])) >= E[64])
    exact = np.array([-1.0, 0.0, 1.0])
    assert label(rows([[1, 0, 1], [1, 0, -1], [1, 0, -1.5], [1, 0, 0.5]]), 1, edges=exact)[1]["bins"].tolist() == [-1, 0, -1, 1]


def test_origin_moves_the_sensor():
    ids, info = label(rows([[11, -2, 3.5], [10, -2, 3.5]]), 1, origin=(10, -2, 3.5), **EDGE_FOV)
    assert info["bins"].tolist() == [48, -1]                 # z == 0 from the origin; the origin itself has rho2 == 0


def test_empty_and_one_point_scenes_and_one_beam():
    ids, info = B.label_beams([np.zeros((0, 4), np.float32), rows([[3, 0, -1]]), rows([[0, 0, 2]])], 4, device="cpu")
    assert [len(i) for i in ids] == [0, 1, 1] and ids[1].tolist() == [0] and ids[2].tolist() == [-1]
    for k in (0, 2):                                         # no assigned point: no cluster
        assert info[k]["clusters"] == 0 and info[k]["iterations"] == 0 and (info[k]["counts"] == 0).all() and (info[k]["table"] == -1).all()
    assert info[1]["clusters"] == 1 and info[1]["counts"].tolist() == [1, 0, 0, 0] and info[1]["iterations"] == 1
    assert B.label_beams([], 4, device="cpu") == ([], [])
    pts, rings = T.wall_ring(3, 8, 50)
    ids, info = label(pts, 1)
    assert (ids == 0).all() and info["counts"].tolist() == [400] and info["iterations"] == 1
    occupied = np.flatnonzero(info["hist"])
    assert info["centres"][0] == (info["hist"][occupied].astype(np.int64) * occupied).sum() / 400.0


def hist_of(counts, bins=32):
    h = np.zeros(bins, dtype=np.uint32)
    for i, c in counts.items():
        h[i] = c
    return h


def test_lloyd_ties_go_to_the_lower_cluster():
    table, centres, counts, iters, flags = B.lloyd(hist_of({10: 3, 20: 5}), 2)
    assert table[[10, 20]].tolist() == [0, 1] and centres.tolist() == [10.0, 20.0] and counts.tolist() == [3, 5] and (iters, flags) == (1, 0)
    table, centres, counts, iters, flags = B.lloyd(hist_of({10: 3, 20: 5}), 3)
    assert table[[10, 20]].tolist() == [0, 2] and centres.tolist() == [10.0, 15.0, 20.0] and counts.tolist() == [3, 0, 5]
    assert (table[np.r_[0:10, 11:20, 21:32]] == -1).all()
    table, centres, counts, _, _ = B.lloyd(hist_of({10: 1, 15: 1, 20: 1}), 2)    # bin 15 is as far from 10 as from 20
    assert table[[10, 15, 20]].tolist() == [0, 0, 1] and centres.tolist() == [12.5, 20.0] and counts.tolist() == [2, 1]
    table, centres, counts, _, _ = B.lloyd(hist_of({10: 1, 11: 1}), 3)           # centres 10, 10.5, 11: nothing is nearer to the middle one
    assert table[[10, 11]].tolist() == [0, 2] and counts.tolist() == [1, 0, 1]
    table, centres, counts, _, _ = B.lloyd(hist_of({7: 9}), 3)                   # one occupied bin: every centre starts on it
    assert table[7] == 0 and centres.tolist() == [7.0, 7.0, 7.0] and counts.tolist() == [9, 0, 0]


def test_lloyd_moves_the_centres_and_counts_its_updates():
    rng = np.random.default_rng(4)
    hist = rng.integers(0, 40, 256).astype(np.uint32) * (rng.random(256) < 0.7)
    table, centres, counts, iters, flags = B.lloyd(hist, 5)
    assert 2 <= iters < B.MAX_ITERS and flags == 0 and (np.diff(centres) > 0).all() and counts.sum() == hist.sum()
    occ = np.flatnonzero(hist)
    assert (np.diff(table[occ]) >= 0).all()                  # clusters are runs of bins
    for k in range(5):                                       # a fixed point: every centre is its cluster's mean, every bin with its nearest centre
        mine = occ[table[occ] == k]
        assert centres[k] == (hist[mine].astype(np.int64) * mine).sum() / float(hist[mine].sum())
    assert np.array_equal(table[occ], np.argmin(np.abs(occ[:, None] - centres[None, :]), axis=1))


def test_unassigned_modes_and_keep_beams():
    pts, rings = T.wall_ring(5, 8, 30)
    pts = np.concatenate([pts, rows([[0, 0, 1], [np.nan, 0, 0]])])               # two unassigned rows at the end
    rings = np.concatenate([rings, [-1, -1]])
    kept, rep = B.resample_scenes([pts], 8, stride=4, phase=1, device="cpu")
    assert kept[0].tobytes() == pts[(rings % 4 == 1) | (rings < 0)].tobytes() and rep[0]["unassigned"] == 2
    kept, rep = B.resample_scenes([pts], 8, stride=4, phase=1, unassigned="drop", device="cpu")
    assert kept[0].tobytes() == pts[(rings >= 0) & (rings % 4 == 1)].tobytes()
    kept, rep = B.resample_scenes([pts], 8, keep_beams=[0, 5, 7], unassigned="drop", device="cpu")
    assert kept[0].tobytes() == pts[np.isin(rings, [0, 5, 7])].tobytes() and rep[0]["kept"] == 90 and rep[0]["points"] == 242


def test_bad_arguments():
    with pytest.raises(ValueError):
        B.edge_table((10.0, -30.0), 64)                      # decreasing
    with pytest.raises(ValueError):
        B.edge_table((-30.0, 100.0), 64)                     # through 90 degrees: the tangent jumps back
    with pytest.raises(ValueError):
        B.edge_table((-30.0, 10.0), B.MAX_BINS + 1)
    with pytest.raises(ValueError):
        B.label_beams([rows([[1, 0, 0]])], 1, device="cpu", edges=[0.0, 1.0, 1.0])
    for kw in (dict(stride=0), dict(stride=2, phase=2), dict(), dict(stride=2, keep_beams=[1]), dict(keep_beams=[8]), dict(stride=-1)):
        with pytest.raises(ValueError):
            B.resample_scenes([rows([[1, 0, 0]])], 8, device="cpu", **kw)
    with pytest.raises(ValueError):
        B.resample_scenes([rows([[1, 0, 0]])], B.MAX_BEAMS + 1, stride=1, device="cpu")
    with pytest.raises(ValueError):
        B.resample_scenes([rows([[1, 0, 0]])], 8, stride=1, unassigned="maybe", device="cpu")
    with pytest.raises(ValueError):
        B.label_beams([rows([[1, 0, 0]])], 8, device="tpu")


# ---- the tool
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("beam") / "src")
    ids, clouds, rings = T.write_tree(root)
    return root, ids, clouds, rings


def test_tool_writes_the_kept_rows_links_and_log(tree, tmp_path):
    src, ids, clouds, rings = tree
    dst = str(tmp_path / "dst")
    results = B.convert_tree(src, dst, T.TREE_BEAMS, stride=2, device="cpu", batch=4, log=quiet)
    assert [i for i, _ in results] == ids
    for i, c, r in zip(ids, clouds, rings):
        with open(os.path.join(dst, "training", "velodyne", i + ".bin"), "rb") as f:
            assert f.read() == c[r % 2 == 0].tobytes(), i
    for sub in ("label_2", "calib", "image_2", "planes"):
        link = os.path.join(dst, "training", sub)
        assert os.path.islink(link) and os.readlink(link) == os.path.join(os.path.abspath(src), "training", sub)
    assert not os.path.islink(os.path.join(dst, "training", "velodyne"))
    for split in ("train", "val", "trainval"):
        assert open(os.path.join(dst, split + ".txt")).read() == open(os.path.join(src, split + ".txt")).read()
    lines = open(os.path.join(dst, B.LOG_NAME)).read().splitlines()
    assert len(lines) == len(ids) + 1
    points = kept = 0
    for line, i, c, r in zip(lines, ids, clouds, rings):
        f = dict(x.split("=") for x in line.split()[1:])
        assert line.split()[0] == i and int(f["points"]) == len(c) and int(f["kept"]) == int((r % 2 == 0).sum())
        assert int(f["unassigned"]) == 0 and int(f["clusters"]) == T.TREE_BEAMS and int(f["iterations"]) >= 1
        points, kept = points + len(c), kept + int(f["kept"])
    assert lines[-1].startswith("6 scenes, beams 16: points %d, kept %d, unassigned 0; 0 scenes hit the cap" % (points, kept))
    before = T.listing(dst)
    with pytest.raises(FileExistsError):                     # a rerun without --overwrite is refused ...
        B.convert_tree(src, dst, T.TREE_BEAMS, stride=2, device="cpu", log=quiet)
    assert T.listing(dst) == before
    B.main([src, dst, "--beams", "16", "--stride", "2", "--device", "cpu", "--overwrite", "--batch", "3"])     # ... with it, it changes nothing
    assert T.listing(dst) == before


def test_tool_split_ids_and_check(tree, tmp_path, capsys):
    src, ids, clouds, rings = tree
    dst = str(tmp_path / "dst")
    got = B.convert_tree(src, dst, T.TREE_BEAMS, keep_beams=[1, 2], split="val", check=True, device="cpu")
    assert not os.path.exists(dst) and [i for i, _ in got] == ids[1::2]
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 4 and out[0].startswith(ids[1] + " points=%d kept=%d " % (len(clouds[1]), 2 * T.TREE_AZIMUTHS[1]))
    B.main([src, dst, "--beams", "16", "--stride", "4", "--phase", "3", "--ids", ids[2], ids[0], "--device", "cpu"])
    assert sorted(os.listdir(os.path.join(dst, "training", "velodyne"))) == [ids[0] + ".bin", ids[2] + ".bin"]
    assert np.fromfile(os.path.join(dst, "training", "velodyne", ids[2] + ".bin"), np.float32).tobytes() == clouds[2][rings[2] % 4 == 3].tobytes()


def test_tool_leaves_what_stands_in_dst_and_never_writes_through_a_link(tree, tmp_path):
    src, ids, clouds, rings = tree
    dst = str(tmp_path / "dst")
    os.makedirs(os.path.join(dst, "training", "velodyne"))
    os.symlink(os.path.join(dst, "nowhere"), os.path.join(dst, "training", "calib"))           # a dangling link
    with open(os.path.join(dst, "training", "planes"), "w") as f:                              # a plain file
        f.write("mine\n")
    source_bin = os.path.join(src, "training", "velodyne", ids[0] + ".bin")
    os.symlink(source_bin, os.path.join(dst, "training", "velodyne", ids[0] + ".bin"))         # a sweep that is a link into SRC
    B.convert_tree(src, dst, T.TREE_BEAMS, stride=2, overwrite=True, device="cpu", log=quiet)
    assert os.readlink(os.path.join(dst, "training", "calib")) == os.path.join(dst, "nowhere")
    assert open(os.path.join(dst, "training", "planes")).read() == "mine\n" and os.path.islink(os.path.join(dst, "training", "label_2"))
    assert open(source_bin, "rb").read() == clouds[0].tobytes()                                # the source sweep is untouched
    out = os.path.join(dst, "training", "velodyne", ids[0] + ".bin")
    assert not os.path.islink(out) and open(out, "rb").read() == clouds[0][rings[0] % 2 == 0].tobytes()


def test_log_warns_of_empty_clusters(tmp_path):
    """--beams above the positions that return (open sky) leaves clusters empty: the summary names the scenes"""
    src = str(tmp_path / "src")
    os.makedirs(os.path.join(src, "training", "velodyne"))
    pts, rings = T.open_sky(2, 16, 100)
    span = int(rings.max() - rings.min() + 1)
    assert span < 16
    pts.tofile(os.path.join(src, "training", "velodyne", "000007.bin"))
    with open(os.path.join(src, "trainval.txt"), "w") as f:
        f.write("000007\n")
    said = []
    B.convert_tree(src, str(tmp_path / "a"), 16, stride=2, check=True, device="cpu", log=said.append)
    assert "1 scenes with empty clusters: 000007 (WARNING" in said[-1]
    B.convert_tree(src, str(tmp_path / "a"), span, stride=2, check=True, device="cpu", log=said.append)
    assert said[-1].endswith("0 scenes with empty clusters")


def test_tool_refuses_before_it_writes(tree, tmp_path, monkeypatch):
    import torch
    src = tree[0]
    dst = str(tmp_path / "never")
    for kw in (dict(stride=0), dict(stride=2, fov=(10.0, -30.0)), dict(stride=2, fov=(-30.0, 100.0)), dict(stride=2, unassigned="x"),
               dict(stride=2, origin=(0, np.nan, 0)), dict(stride=1, beams=0)):
        kw = dict(dict(beams=T.TREE_BEAMS, device="cpu", log=quiet), **kw)
        with pytest.raises(ValueError):
            B.convert_tree(src, dst, **kw)
    with pytest.raises(ValueError):
        B.convert_tree(src, src, T.TREE_BEAMS, stride=2, overwrite=True, device="cpu", log=quiet)       # never onto the source
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(B.ResampleDeviceError):
        B.main([src, dst, "--beams", "16", "--stride", "2"])
    with pytest.raises(B.ResampleDeviceError):
        B.label_beams([rows([[1, 0, 0]])], 1, device="cuda")
    with pytest.raises(B.ResampleDeviceError):
        B.resample_scenes([rows([[1, 0, 0]])], 1, stride=1, device="cuda:0")
    assert not os.path.exists(dst)
