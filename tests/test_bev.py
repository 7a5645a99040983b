"""CPU tests of the BEV renderer (3d_adapt_auto_driving_amd/bev.py): the numpy definition against the reference's own
get_object_mask (tests/golden/g27_bev_mask_ref.npz, tests/golden/make_golden_bev.py) and against hand-written known answers, View's
validation, the argument checks of the two C entries, and both commands on a tiny tree (tests/bev_tree.py)."""
import os

import numpy as np
import pytest

from conftest import pkg
import bev_tree


def bev():
    return pkg("bev")


@pytest.fixture(scope="module")
def g27():
    return dict(np.load(bev_tree.G27, allow_pickle=False))


def g27_cases(g):
    """-> [(name, velo, Calib, Car / Van objects, the reference's mask)]"""
    SN = pkg("stat_norm")
    calib = SN.Calib(SN.parse_calib(str(g["calib_text"])))
    out = []
    for c in ("src", "dst"):
        for s in (0, 1):
            objs = [SN.Object3d(line) for line in str(g["labels_%s_%d" % (c, s)]).split("\n")]
            out.append(("%s_%d" % (c, s), g["velo_%s_%d" % (c, s)], calib, [o for o in objs if o.cls_type in ("Car", "Van")],
                        g["mask_%s_%d" % (c, s)]))
    return out


def identity_calib():
    SN = pkg("stat_norm")
    return SN.Calib({"P2": np.zeros(12), "Tr_velo_to_cam": np.eye(3, 4).ravel(), "R0_rect": np.eye(3).ravel()})


def pixel_set(mask):
    return {(int(r), int(c)) for r, c in zip(*np.nonzero(mask))}


def picture(rows):
    """'#' marks -> the set of (row, col)"""
    return {(r, c) for r, line in enumerate(rows) for c, ch in enumerate(line) if ch == "#"}


def test_checker_mask_equals_the_reference(g27):
    B = bev()
    for name, velo, calib, objs, want in g27_cases(g27):
        got = B.object_mask(velo, calib, objs, device="cpu")
        assert got.dtype == bool and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int(np.sum(got != want)))
        assert 300 < int(want.sum()) < len(want)
    labels = str(g27["labels_src_0"])
    assert "Pedestrian" in labels and "DontCare" in labels and "Van" in labels


def test_fixture_is_small():
    assert os.path.getsize(bev_tree.G27) < 200 * 1024


# ---- outlines: the exact pixel sets of one horizontal and one diagonal segment
HORIZONTAL = [12, 20, 52, 20]                    # centre of (row 2, col 1) -> centre of (row 2, col 6)
DIAGONAL = [12, 52, 52, 12]                      # centre of (row 6, col 1) -> centre of (row 1, col 6)
WANT_SEGMENTS = {
    1: (picture(["........",
                 "........",
                 ".######.",
                 "........",
                 "........",
                 "........",
                 "........",
                 "........"]),
        picture(["........",
                 "......#.",
                 ".....#..",
                 "....#...",
                 "...#....",
                 "..#.....",
                 ".#......",
                 "........"])),
    # R = 12 units = 1.5 pixels: the horizontal line's neighbours 8 units away, and its caps (8, 8) away (128 <= 144);
    # the diagonals at 8 / sqrt(2) = 5.66 and 11.31 units, not the ones at 16.97
    3: (picture(["........",
                 "########",
                 "########",
                 "########",
                 "........",
                 "........",
                 "........",
                 "........"]),
        picture([".....###",
                 "....####",
                 "...#####",
                 "..#####.",
                 ".#####..",
                 "#####...",
                 "####....",
                 "###....."])),
}


def segment_images(line_px, device):
    B = bev()
    view = B.View((0, 8), (0, 8), 1.0, line_px)
    segs = [np.array([HORIZONTAL + [B.OUTLINE_ROW]], np.int32), np.array([DIAGONAL + [B.OUTLINE_ROW + 1]], np.int32)]
    return B.compose(np.zeros((2, 3, 8, 8), np.uint32), segs, view, device=device)


@pytest.mark.parametrize("line_px", (1, 3))
def test_segment_pixels_known_answer(line_px):
    B = bev()
    rgb = segment_images(line_px, "cpu")
    assert rgb.shape == (2, 8, 8, 3) and rgb.dtype == np.uint8
    for k in range(2):
        on = (rgb[k] == B.PALETTE[B.OUTLINE_ROW + k]).all(-1)
        assert pixel_set(on) == WANT_SEGMENTS[line_px][k], (line_px, k)
        assert (rgb[k][~on] == B.PALETTE[0]).all()


# ---- binning: the edges of the frame
def edge_cloud():
    """x = x0, x = x1, just inside both, z = z0, z = z1, NaN; view x (0, 4), z (0, 4), res 0.5 -> 8 x 8.  (The smallest steps are
    normal numbers: 1e-30, not a denormal.)"""
    f = np.float32
    return np.array([[0.0, 0, 1.25, 0],                                  # x = x0: u = 0, kept, col 0; v = 2.5 -> row 7 - 2 = 5
                     [4.0, 0, 1.25, 0],                                  # x = x1: u = 8 = W, dropped
                     [1e-30, 0, 1.25, 0],                                # just inside x0: col 0
                     [np.nextafter(f(4), f(0)), 0, 1.25, 0],             # just inside x1: u = 7.9999995, col 7
                     [-1e-30, 0, 1.25, 0],                               # just outside x0: u < 0, dropped
                     [2.75, 0, 0.0, 0],                                  # z = z0: row 7, col 5
                     [2.75, 0, 4.0, 0],                                  # z = z1: dropped
                     [2.75, 0, np.nextafter(f(4), f(0)), 0],             # just inside z1: row 0
                     [np.nan, 0, 1.0, 0], [1.0, 0, np.nan, 0], [1.0, np.nan, 1.0, 0]], dtype=np.float32)


def test_binning_edges_known_answer():
    B = bev()
    view = B.View((0, 4), (0, 4), 0.5)
    assert (view.width, view.height) == (8, 8) and view.inv == np.float32(2)
    counts, cls, stats = B.bin_points([B.Cloud(edge_cloud(), identity_calib(), np.zeros((0, 7)), 0, 1)], [0], 1, view, device="cpu")
    want = np.zeros((1, 3, 8, 8), np.uint32)
    want[0, 0, 5, 0] = 2
    want[0, 0, 5, 7] = 1
    want[0, 0, 7, 5] = 1
    want[0, 0, 0, 5] = 1
    assert counts.dtype == np.uint32 and np.array_equal(counts, want)
    assert stats.tolist() == [[[5, 6], [0, 0], [0, 0]]]
    assert cls[0].tolist() == [0] * 11


def test_mask_is_strict_and_layers_follow_it():
    B = bev()
    view = B.View((-4, 4), (0, 8), 1.0)
    box = np.array([[0.0, 1.0, 4.0, 2.0, 2.0, 4.0, 0.0]])              # x in (-2, 2), y in (-1, 1), z in (3, 5)
    pts = np.array([[0, 0, 4, 0], [2, 0, 4, 0], [-2, 0, 4, 0], [1.5, 1, 4, 0], [1.5, -1, 4, 0], [1.5, 0.5, 3, 0], [1.5, 0.5, 4.5, 0],
                    [np.nan, 0, 4, 0]], np.float32)
    want = [True, False, False, False, False, False, True, False]
    assert B.object_mask(pts, identity_calib(), box, device="cpu").tolist() == want
    counts, cls, stats = B.bin_points([B.Cloud(pts, identity_calib(), box, 0, 2)], [0], 1, view, device="cpu")
    assert cls[0].tolist() == [int(w) for w in want]
    assert stats.tolist() == [[[5, 1], [0, 0], [2, 0]]]
    assert counts[0, 2, 3, 4] == 1 and counts[0, 2, 3, 5] == 1 and counts[0, 2].sum() == 2 and counts[0, 1].sum() == 0
    # a layer byte of NOT_DRAWN takes the point out of the image and out of the stats
    counts, _, stats = B.bin_points([B.Cloud(pts, identity_calib(), box, B.NOT_DRAWN, 2)], [0], 1, view, device="cpu")
    assert stats.tolist() == [[[0, 0], [0, 0], [2, 0]]] and counts.sum() == 2


def test_brightness_steps_known_answer():
    B = bev()
    ns = [1, 2, 3, 4, 7, 8, 1000]
    view = B.View((0, 1), (0, 1), 1.0)
    counts = np.zeros((len(ns), 3, 1, 1), np.uint32)
    counts[:, 1, 0, 0] = ns
    rgb = B.compose(counts, [np.zeros((0, 5), np.int32)] * len(ns), view, device="cpu")
    for k, step in enumerate([0, 1, 1, 2, 2, 3, 3]):
        assert rgb[k, 0, 0].tolist() == B.PALETTE[1 + 4 * 1 + step].tolist(), ns[k]
    # the same through both stages: 1000 duplicates of one point
    pts = np.tile(np.array([[0.5, 0, 0.5, 0]], np.float32), (1000, 1))
    img, st = B.render_scenes([B.Scene([B.Cloud(pts, identity_calib(), np.zeros((0, 7)), 0, 1)], [])], view, device="cpu")
    assert img[0, 0, 0].tolist() == B.PALETTE[1 + 3].tolist() and st["binned"].tolist() == [[1000, 0, 0]]


def test_precedence_of_layers_and_outlines():
    B = bev()
    view = B.View((0, 6), (0, 1), 1.0)
    counts = np.zeros((1, 3, 1, 6), np.uint32)
    counts[0, 0, 0, 1:] = 1                                              # columns: none | 0 | 0 1 | 0 1 2 | 0 1 2 + outline | + two
    counts[0, 1, 0, 2:] = 2
    counts[0, 2, 0, 3:] = 4
    dot = lambda c, row: [8 * c + 4, 4, 8 * c + 4, 4, row]               # a zero-length segment on the centre of column c
    segs = [np.array([dot(4, B.OUTLINE_ROW + 1), dot(5, B.OUTLINE_ROW + 2), dot(5, B.OUTLINE_ROW)], np.int32)]
    rgb = B.compose(counts, segs, view, device="cpu")[0, 0]
    want = [0, 1, 1 + 4 + 1, 1 + 8 + 2, B.OUTLINE_ROW + 1, B.OUTLINE_ROW]       # the LAST segment in list order wins
    assert rgb.tolist() == B.PALETTE[want].tolist()
    with pytest.raises(ValueError, match="ascending"):
        B.render_scenes([B.Scene([], [(1, np.zeros((0, 7))), (0, np.zeros((0, 7)))])], view, device="cpu")


def test_box_segments_skipped_box_and_zero_size_box():
    B = bev()
    view = B.View((0, 8), (0, 8), 1.0, 1)
    far = np.array([[5000.0, 1.6, 4.0, 1.5, 1.6, 3.9, 0.3], [np.nan, 1.6, 4.0, 1.5, 1.6, 3.9, 0.3]])
    rows, skipped = B.box_segments(far, view, 0)
    assert rows.shape == (0, 5) and skipped == 2
    # heading: the front is at centre + l/2 (cos ry, -sin ry); ry = 0 -> +x; rows are measured downward from z1
    rows, skipped = B.box_segments(np.array([[4.0, 1.6, 4.0, 1.5, 2.0, 4.0, 0.0]]), view, 1)
    assert skipped == 0 and rows.tolist() == [[48, 24, 48, 40, 14], [48, 40, 16, 40, 14], [16, 40, 16, 24, 14], [16, 24, 48, 24, 14],
                                              [32, 32, 48, 32, 14]]
    zero = np.array([[3.5, 1.6, 4.5, 0.0, 0.0, 0.0, 0.7]])              # the centre of pixel (row 3, col 3)
    for line_px, want in ((1, {(3, 3)}), (3, {(r, c) for r in (2, 3, 4) for c in (2, 3, 4)})):
        v = B.View((0, 8), (0, 8), 1.0, line_px)
        img, st = B.render_scenes([B.Scene([], [(0, zero), (2, far)])], v, device="cpu")
        assert pixel_set((img[0] == B.PALETTE[B.OUTLINE_ROW]).all(-1)) == want
        assert st["skipped_boxes"].tolist() == [2] and st["segments"].tolist() == [5]


def test_view_validation():
    B = bev()
    v = B.View()
    assert (v.width, v.height, v.line_px) == (800, 800, 1)
    for bad in (dict(x_range=(0, 1.05), res=0.1), dict(z_range=(0, 0)), dict(z_range=(5, 1)), dict(res=0.0), dict(res=-1.0),
                dict(x_range=(0, 204.9), res=0.1), dict(z_range=(0, 2049), res=1.0), dict(line_px=0), dict(line_px=9),
                dict(line_px=1.5), dict(x_range=(0, np.inf))):
        with pytest.raises(ValueError):
            B.View(**bad)
    assert B.View((0, 2048), (0, 1), 1.0, 8).width == 2048
    assert B.View((0.0, 0.3), (0.0, 0.7), 0.1).width == 3              # 0.3 / 0.1 is 2.9999999999999996: integral within 1e-6
    assert B.PALETTE.dtype == np.uint8 and B.PALETTE.shape == (16, 3) and len({tuple(r) for r in B.PALETTE.tolist()}) == 16


def test_c_entries_reject_bad_arguments_without_gpu():
    L = pkg("_lib")
    ptrs = [None] * 13                                               # 12 arrays and the stream
    for sizes in ((1, 1, 1, 0, 8), (1, 1, 1, 8, 2049), (-1, 1, 1, 8, 8), (1, 1, -1, 8, 8), (1, -1, 1, 8, 8)):
        with pytest.raises(L.PrcnnError, match="bad sizes"):
            L.call("prcnn_bev_bin", *sizes, 0.0, 0.0, 1.0, *ptrs)
    with pytest.raises(L.PrcnnError, match="null pointer"):
        L.call("prcnn_bev_bin", 1, 1, 1, 8, 8, 0.0, 0.0, 1.0, *ptrs)
    for args in ((-1, 8, 8, 1, 16), (1, 0, 8, 1, 16), (1, 8, 4096, 1, 16), (1, 8, 8, 0, 16), (1, 8, 8, 9, 16), (1, 8, 8, 1, 3),
                 (1, 8, 8, 1, 65)):
        with pytest.raises(L.PrcnnError, match="bad sizes"):
            L.call("prcnn_bev_compose", *args, None, None, None, None, None, None)
    with pytest.raises(L.PrcnnError, match="null pointer"):
        L.call("prcnn_bev_compose", 1, 8, 8, 1, 16, None, None, None, None, None, None)


# ---- the commands on a tiny tree
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return bev_tree.make_tree(str(tmp_path_factory.mktemp("bev_tree")))


def decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


VIEW_ARGS = ["--x_range", "-10", "10", "--z_range", "0", "20", "--res", "0.125"]


def test_cuda_without_a_device_raises_before_writing(tree, tmp_path, monkeypatch):
    import torch
    B = bev()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = tmp_path / "never"
    with pytest.raises(B.RenderDeviceError):
        B.main(["compare", tree[0], tree[1], "--split", "trainval", "--out_dir", str(out), "--device", "cuda"] + VIEW_ARGS)
    with pytest.raises(B.RenderDeviceError):
        B.main(["scene", tree[0], "--ids", "0", "--out_dir", str(out)] + VIEW_ARGS)
    assert not out.exists()
    with pytest.raises(B.RenderDeviceError):
        B.object_mask(np.zeros((4, 4), np.float32), identity_calib(), np.zeros((0, 7)), device="cuda")
    with pytest.raises(ValueError):
        B.render_scenes([], B.View(), device="tpu")


def test_compare_command_cpu(tree, tmp_path, capsys):
    B = bev()
    out = tmp_path / "cmp"
    images = B.main(["compare", tree[0], tree[1], "--split", "trainval", "--out_dir", str(out), "--device", "cpu", "--batch", "2"]
                    + VIEW_ARGS)
    lines = capsys.readouterr().out.strip().split("\n")
    assert sorted(images) == bev_tree.IDS and len(lines) == 3 and lines[0].startswith("000000  layer0 ")
    layer = lambda img, l: np.isin(img.astype(np.int64) @ [65536, 256, 1], B.PALETTE[1 + 4 * l:5 + 4 * l].astype(np.int64) @ [65536, 256, 1])
    for i in bev_tree.IDS:
        img = images[i]
        assert img.shape == (160, 160, 3) and np.array_equal(decoded(str(out / (i + ".png"))), img)
        before, after = layer(img, 1), layer(img, 2)
        assert after.any() and before.any() and not np.array_equal(after, before)      # the rescaled cars cover other pixels
        assert layer(img, 0).any()
        for g in (0, 1):
            assert (img == B.PALETTE[B.OUTLINE_ROW + g]).all(-1).any()
    assert " layer2 " in lines[0] and "dropped" in lines[0] and "skipped_boxes 0" in lines[0]
    # --ids and --limit select; a pedestrian is no object point of the default classes
    one = B.main(["compare", tree[0], tree[1], "--ids", "1", "--out_dir", str(tmp_path / "one"), "--device", "cpu"] + VIEW_ARGS)
    assert list(one) == ["000001"] and np.array_equal(one["000001"], images["000001"])
    two = B.main(["compare", tree[0], tree[1], "--split", "trainval", "--limit", "2", "--out_dir", str(tmp_path / "two"), "--device",
                  "cpu"] + VIEW_ARGS)
    assert list(two) == bev_tree.IDS[:2]


def test_scene_command_cpu(tree, tmp_path, capsys):
    B = bev()
    out = tmp_path / "scene"
    images = B.main(["scene", tree[0], "--split", "trainval", "--out_dir", str(out), "--result_dir", tree[2], "--device", "cpu",
                     "--line_px", "2"] + VIEW_ARGS)
    capsys.readouterr()
    det = lambda img: int((img == B.PALETTE[B.OUTLINE_ROW + 2]).all(-1).sum())
    for i in bev_tree.IDS:
        assert np.array_equal(decoded(str(out / (i + ".png"))), images[i])
        assert (images[i] == B.PALETTE[B.OUTLINE_ROW]).all(-1).any()
        assert not (images[i] == B.PALETTE[B.OUTLINE_ROW + 1]).all(-1).any() and not (images[i] == B.PALETTE[9:13][:, None, None]).all(-1).any()
    assert det(images["000000"]) > 0 and det(images["000001"]) > 0 and det(images["000002"]) == 0      # no result file: no detections
    # the van's detection is below the threshold with the default classes filtered anyway; with it lowered and Van listed it shows
    more = B.main(["scene", tree[0], "--ids", "0", "--out_dir", str(tmp_path / "more"), "--result_dir", tree[2], "--score_thresh", "0.1",
                   "--classes", "Car,Van", "--device", "cpu", "--line_px", "2"] + VIEW_ARGS)
    assert det(more["000000"]) > det(images["000000"])
    none = B.main(["scene", tree[0], "--ids", "0", "--out_dir", str(tmp_path / "none"), "--device", "cpu"] + VIEW_ARGS)
    assert det(none["000000"]) == 0
