"""Microbench of csrc/rcnn_entrance.hip and csrc/rows_layer.hip at the RCNN size of one batch (8 scenes x 100 RoIs x 512 points), and of
the list layer at the engine's shape."""
import importlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
pkg = importlib.import_module("3d_adapt_auto_driving_amd"); sys.path.insert(0, pkg.DROPIN_DIR)
import pointnet2_cuda as P
dev = torch.device("cuda", 0)
R, ld = 409600, 136
g = torch.Generator(device=dev).manual_seed(0)
rows = torch.randn((R, ld), device=dev, generator=g)
W = lambda *s: torch.randn(s, device=dev, generator=g) / s[0] ** 0.5
wu1, wu2, wm, wp = W(8, 128), W(128, 128), W(256, 128), W(128, 128)
b = [torch.randn(128, device=dev, generator=g) * 0.1 for _ in range(4)]
xfeat, merged, p = (torch.empty((R, 128), device=dev) for _ in range(3))
run = lambda: P.rcnn_point_mlp_wrapper(rows, 8, wu1, b[0], wu2, b[1], wm, b[2], wp, b[3], xfeat, merged, p)
for _ in range(3): run()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(10): run()
torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 100
print("rcnn_point_mlp: %.3f ms per call (%.1f TFLOP/s over 53.7 GFLOP)" % (ms, 2 * R * (128 * 128 * 4) / ms / 1e9))
# the fused entrance kernel (only P leaves the CU): every tile, and the live tiles of a step (a RoI holds ~54 of its 512 rows)
def timed(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e6
p2 = torch.empty((R, 128), device=dev)
us = timed(lambda: P.rcnn_point_mlp_wrapper(rows, 8, wu1, b[0], wu2, b[1], wm, b[2], wp, b[3], None, None, p2))
print("rcnn_entrance, all 6400 tiles : %.1f us (%.1f TFLOP/s)" % (us, 2 * R * (128 * 128 * 4) / us / 1e6))
assert torch.equal(p2, p), "fused entrance != three launches"
cnt = torch.from_numpy(np.random.default_rng(0).poisson(54, 800).clip(1, 512).astype(np.int32)).to(dev)
tiles = P.pooled_tiles_wrapper(cnt, 512)
us = timed(lambda: P.rcnn_point_mlp_wrapper(rows, 8, wu1, b[0], wu2, b[1], wm, b[2], wp, b[3], None, None, p2, tiles))
print("rcnn_entrance, live tiles of a step (~1.3 per RoI): %.1f us" % us)
# the 128-wide layer over a row list (rows_layer_list_kernel) at the engine's shape: the per-point part of the RCNN's second SA level over
# 1600 RoI clouds x 128 level-1 centres, of which a RoI lists the ~47 that are their own representatives (the uniform scene's share)
clouds, per = 1600, 128
cnt2 = torch.from_numpy(np.random.default_rng(1).poisson(47, clouds).clip(1, per).astype(np.int32)).to(dev)
rowlist = P.pooled_rows_wrapper(cnt2, per)
a2 = torch.randn((clouds * per, 128), device=dev, generator=g)
o2 = torch.empty((clouds * per, 128), device=dev)
us = timed(lambda: P.rows_gemm128_rows_wrapper(a2, wp, b[3], False, o2, rowlist), 50)
print("rows_gemm128_rows, %d of %d rows listed: %.1f us" % (int(rowlist[1][1]), clouds * per, us))
