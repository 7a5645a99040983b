/*
 * prcnn_hip.h -- C ABI of libprcnn_hip.so: the MI355X (gfx950) implementation of the
 * PointRCNN eval_rcnn hot-path operators of cxy1997/3D_adapt_auto_driving.
 *
 * This is the drop-in boundary.  Every entry point is what the reference's three pybind
 * modules bind for this path (reference paths relative to /root/reference/pointrcnn/):
 *
 *   pointnet2_cuda  pointnet2_lib/pointnet2/src/pointnet2_api.cpp:10-24
 *   iou3d_cuda      lib/utils/iou3d/src/iou3d.cpp:174-179
 *   roipool3d_cuda  lib/utils/roipool3d/src/roipool3d.cpp:198-203
 *   rotate_iou      ../evaluate/rotate_iou.py:294-329 (numba.cuda kernel :261-291)
 *
 * Conventions (same as the reference wrappers):
 *   - plain device pointers + sizes; f32 / i32, C-contiguous, row-major; the CALLER allocates
 *     every output; dims are passed as ints.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  The
 *     reference launches pointnet2 on torch's current stream and iou3d/roipool3d on the default
 *     stream; here every op takes the stream explicitly and is asynchronous unless stated.
 *   - return value: 0 on success, a negative PRCNN_E* code on failure (the reference calls
 *     exit(-1) on a failed launch, ball_query_gpu.cu:63-66; we report instead).
 *     prcnn_last_error() returns a static description of the last failure on this thread.
 *   - no allocation inside any call except the blocking prcnn_nms / prcnn_nms_normal, which
 *     keep one cached device scratch (the reference cudaMalloc/cudaFree's per call,
 *     iou3d.cpp:87,97).
 */
#ifndef PRCNN_HIP_H
#define PRCNN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PRCNN_OK 0
#define PRCNN_EINVAL (-1)  /* bad argument (null pointer, negative size, unsupported size) */
#define PRCNN_ELAUNCH (-2) /* HIP launch / runtime error */

int prcnn_version(void);
const char *prcnn_last_error(void);
/* opt_n_threads() of cuda_utils.h:10-13: the reference FPS block size for n points. */
int prcnn_opt_n_threads(int work_size);

/* ---- pointnet2_cuda ------------------------------------------------------------------ */

/* ball_query_wrapper_fast  src/ball_query.cpp:14-25 -> kernel src/ball_query_gpu.cu:9-45.
 * new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample): first nsample in-radius indices in index
 * order, first hit back-fills; rows of empty balls are left untouched (caller zero-fills). */
int prcnn_ball_query(int b, int n, int m, float radius, int nsample,
                     const float *new_xyz, const float *xyz, int *idx, void *stream);

/* prcnn_ball_query with EVERY slot of idx written: the row of an empty ball holds the zeros the reference's caller fills the tensor
 * with first (pointnet2_utils.py:218) -- the engine's form (no fill launch in front of each query). */
int prcnn_ball_query_full(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                          void *stream);

/* Algorithm selector for ball query (results are identical): 0 = automatic (bucket-sorted hashed grid with a
 * wave per centre for n >= 2048 points -- csrc/ball_dense.hip --, brute-force scan otherwise), 1 = brute-force
 * scan only, 2 = round 1's linked-list hashed grid (n >= 4096) in place of the bucket-sorted one.  For tests /
 * profiling. */
int prcnn_set_ball_query_mode(int mode);

/* group_points_wrapper_fast  src/group_points.cpp:25-36 -> src/group_points_gpu.cu:47-66.
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample). */
int prcnn_group_points(int b, int c, int n, int npoints, int nsample,
                       const float *points, const int *idx, float *out, void *stream);
/* group_points_grad_wrapper_fast  src/group_points.cpp:11-22 -> src/group_points_gpu.cu:8-25.
 * grad_points (b,c,n) must be zero-filled by the caller; atomic scatter-add. */
int prcnn_group_points_grad(int b, int c, int n, int npoints, int nsample,
                            const float *grad_out, const int *idx, float *grad_points, void *stream);

/* Ball query over clouds whose points k >= limit[cloud] are copies of point k % limit[cloud] (the pooled rows of a RoI that
 * holds fewer than 512 points, roipool3d_kernel.cu:152-159): only the first limit[cloud] points are scanned.  Same distinct
 * points per ball as prcnn_ball_query, slots past them repeat the first hit; every slot of idx is written (an empty ball gets
 * zeros).  Engine-side shortcut, not reference ABI. */
int prcnn_ball_query_limit(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                           const int *limit, int *idx, void *stream);

/* gather_points_wrapper_fast  src/sampling.cpp:11-20 -> src/sampling_gpu.cu:8-24. */
int prcnn_gather_points(int b, int c, int n, int npoints,
                        const float *points, const int *idx, float *out, void *stream);
/* gather_points_grad_wrapper_fast  src/sampling.cpp:23-33 -> src/sampling_gpu.cu:46-63. */
int prcnn_gather_points_grad(int b, int c, int n, int npoints,
                             const float *grad_out, const int *idx, float *grad_points, void *stream);

/* furthest_point_sampling_wrapper  src/sampling.cpp:36-46 -> src/sampling_gpu.cu:93-253.
 * xyz (b,n,3), temp (b,n) scratch pre-filled by the caller (1e10) -> idx (b,m).  Ties resolve
 * as in the reference kernel launched with opt_n_threads(n) threads.  On return temp holds the
 * running minimum distances, as the reference leaves them. */
int prcnn_furthest_point_sampling(int b, int n, int m,
                                  const float *xyz, float *temp, int *idx, void *stream);

/* Which ARITHMETIC the squared distance of sampling_gpu.cu:133 is evaluated in, for every FPS entry point of the library
 * (process-wide, read at launch).  0 (default): the source's -- (dx*dx + dy*dy) + dz*dz, one rounding per operation: the parity
 * contract of this build, independent of any compiler's contraction choices.  1: the reference's KERNEL BINARY as hipcc builds
 * that file for gfx950 -- (fma(dy, dy, dx*dx)) + dz*dz, read off its disassembly: a user who migrates from the hipcc-compiled
 * reference and wants its picks bit for bit (near-ties included) selects this one.  (What nvcc made of the expression on the
 * reference's original platform is not observable here; oracle/fma_table.py counts how rarely any contraction moves a pick.) */
int prcnn_set_fps_arithmetic(int mode);

/* FPS with the selected points' coordinates written beside their indices: the result of furthest_point_sample + gather_operation
 * (pointnet2_modules.py:40-46) in one launch (no scratch fill, index cast or gather by the caller).  Served shapes: n <= 1024 (many small
 * clouds, a wave or four per cloud) and, since round 4, 2048 < n <= 16384 with m >= 256 (the speculative kernel; round 5: 16384 < n <= 32768 on two workgroups per cloud, and every other shape through an internal distance scratch + gather).  Same selection, same
 * tie rule as prcnn_furthest_point_sampling. */
int prcnn_fps_new_xyz(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream);

/* prcnn_fps_new_xyz for a caller that expects the answer to be the prefix 0 .. m-1: xyz is the new_xyz of an earlier sampling of a
 * larger cloud (its picks in pick order), as at every level but the first of a set-abstraction pyramid.  Furthest point sampling is a
 * greedy arg-max, hence prefix-consistent up to exact ties at a maximum; the library checks that per cloud in parallel (n * m distance
 * evaluations, no dependent chain), writes the prefix for the clouds that pass and runs the sampling kernels for the others in the
 * same launches.  SAME outputs as prcnn_fps_new_xyz for ANY input -- the hint only says the check is worth running.  Shapes outside
 * prcnn_fps_nested_supported (1: 2 <= m <= n <= 16384) go to prcnn_fps_new_xyz unchanged. */
int prcnn_fps_new_xyz_nested(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream);
int prcnn_fps_nested_supported(int n, int m);
/* The check alone: rejected (b) <- 0 where sampling m of the cloud's n points returns 0 .. m-1 (decided with the arithmetic of
 * prcnn_set_fps_arithmetic and the tie order of prcnn_furthest_point_sampling), 1 where it may not; idx (b,m) / new_xyz (b,m,3), each
 * NULL or written with the prefix for every cloud.  b <= 65535, shapes: prcnn_fps_nested_supported. */
int prcnn_fps_prefix_check(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, int *rejected, void *stream);
/* The sampling launches of prcnn_fps_new_xyz_nested alone, under a caller-made verdict (a test hook): clouds with rejected[c] == 0 are
 * left untouched in idx / new_xyz, the others are sampled as by prcnn_fps_new_xyz.  Shapes: prcnn_fps_nested_supported.  Where the
 * coordinates are gathered behind the sampling (n > 1024 outside the speculative kernel's range) a skipped cloud's idx must hold valid
 * indices: its new_xyz is gathered from them. */
int prcnn_fps_new_xyz_flagged(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, const int *rejected, void *stream);

/* three_nn_wrapper_fast  src/interpolate.cpp:14-23 -> src/interpolate_gpu.cu:9-52.
 * unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) SQUARED distances, idx (b,n,3). */
int prcnn_three_nn(int b, int n, int m, const float *unknown, const float *known,
                   float *dist2, int *idx, void *stream);

/* three_nn followed by the weights of PointnetFPModule.forward (pointnet2_lib/pointnet2/pointnet2_modules.py:139-144;
 * pointnet2_utils.py:97 takes the square root) in the kernel's epilogue: idx (b,n,3) i32, weight (b,n,3) f32 with
 * r_k = 1 / (sqrt(dist2_k) + 1e-8), weight_k = r_k / ((r_0 + r_1) + r_2), one rounding per operation.  The engine's form: the
 * reference's Python runs this as sqrt, add, reciprocal, sum, divide -- five launches per FP level. */
int prcnn_three_nn_weights(int b, int n, int m, const float *unknown, const float *known, int *idx, float *weight,
                           void *stream);
/* three_interpolate_wrapper_fast  src/interpolate.cpp:26-39 -> src/interpolate_gpu.cu:77-97.
 * points (b,c,m), idx/weight (b,n,3) -> out (b,c,n). */
int prcnn_three_interpolate(int b, int c, int m, int n, const float *points,
                            const int *idx, const float *weight, float *out, void *stream);
/* three_interpolate_grad_wrapper_fast  src/interpolate.cpp:42-54 -> interpolate_gpu.cu:120-142. */
int prcnn_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                                 const int *idx, const float *weight, float *grad_points, void *stream);

/* Fused QueryAndGroup.forward (pointnet2_utils.py:241-264 = K1 + K2 x2 + centre subtract + cat):
 * out (b,3+c,m,nsample) = cat(xyz[idx]-new_xyz, features[idx]); features may be NULL (c = 0).
 * idx (b,m,nsample) is an OUTPUT here and is fully written (empty balls -> 0, the value the
 * reference's zero-filled idx holds).  Not part of the reference ABI; it is what the
 * reference's Python composes from it. */
int prcnn_query_and_group(int b, int n, int m, int c, float radius, int nsample,
                          const float *new_xyz, const float *xyz, const float *features,
                          int *idx, float *out, void *stream);

/* ---- the order-fixed backward of grouping, gather and three_interpolate (csrc/scatter_plan.hip; not in the
 *      reference ABI).  The three gradients above are scatter-adds through float atomics: the order of a destination's sum is arrival
 *      order.  Here the index is transposed once per call and every destination sums its own list in a fixed order: no atomics on
 *      floats, the same input gives the same bits. ------------------------------------------------------------------------------- */

/* The transposed index ("scatter plan") of idx (b,slots) i32 over n destinations per cloud -- any of the three operators' index
 * tensors, flattened per cloud: (b, npoint*nsample), (b, npoint) or (b, 3*n_unknown):
 *   offsets (b,n+1) i32: offsets[i][k+1] - offsets[i][k] = the number of slots s with idx[i][s] == k;
 *   entries (b,slots) i32: entries[i][offsets[i][k] .. offsets[i][k+1]) = those slots in ASCENDING order (per cloud the stable argsort
 *   of idx[i], restricted to the values in range); what lies behind offsets[i][n] is unspecified.
 * A slot whose value lies outside [0, n) belongs to no list; nothing is read or written out of bounds for any index content.  A pure
 * function of idx.  No host read and no allocation: work holds prcnn_scatter_plan_workspace(b, n, slots) i32 words (contents
 * arbitrary on entry), so the call is safe on any stream and under graph capture.  b <= 65535, b * n < 2^31. */
int prcnn_scatter_plan_workspace(int b, int n, int slots);
int prcnn_scatter_plan(int b, int n, int slots, const int *idx, int *offsets, int *entries, int *work, void *stream);

/* The ordered sums over a plan.  ARITHMETIC CONTRACT: a destination's list is cut into consecutive chunks of PRCNN_SCATTER_CHUNK
 * entries; each chunk is summed left to right in f32 starting from +0.0f; the chunk sums are then added left to right starting from
 * +0.0f (one rounding per operation, no fma).  EVERY element of grad_points is written -- an empty list gives +0.0f -- so the caller
 * does not zero-fill.  (The chunk rule lets an implementation split a long list over waves and combine the partials in chunk order;
 * it obliges none to.  A cloud with every slot on one point is summed correctly; its speed is no goal.) */
enum { PRCNN_SCATTER_CHUNK = 256 };
/* grad_points (b,c,n)[i][ch][k] = ordered sum over s in list k of grad_out (b,c_total,slots)[i][c0 + ch][s]: the gradient of
 * prcnn_group_points (slots = npoints * nsample, c_total = c, c0 = 0), of the feature channels of prcnn_query_and_group (its whole
 * output gradient with c_total = 3 + c, c0 = 3: nothing is copied) and of prcnn_gather_points (slots = npoints). */
int prcnn_group_points_grad_ordered(int b, int c, int n, int slots, int c_total, int c0, const float *grad_out, const int *offsets,
                                    const int *entries, float *grad_points, void *stream);
/* The gradient of prcnn_three_interpolate: grad_out (b,c,n), weight (b,n,3), the plan of idx (b,3*n) over m destinations -- slot s is
 * unknown point s / 3, neighbour s % 3 -- -> grad_points (b,c,m)[i][ch][k] = ordered sum over s in list k of the f32 product
 * grad_out[i][ch][s / 3] * weight[i][s]. */
int prcnn_three_interpolate_grad_ordered(int b, int c, int n, int m, const float *grad_out, const float *weight, const int *offsets,
                                         const int *entries, float *grad_points, void *stream);

/* ---- the order-fixed TRAINING layer: forward and backward of a 1x1 convolution, BatchNorm on batch statistics and ReLU
 *      (pytorch_utils.Conv1d / Conv2d in training mode; csrc/train_layer.hip; not in the reference ABI).
 *      x (b,cin,p) f32, w (cout,cin), z / y / dz (b,cout,p): torch's layout, p = N of a Conv1d block or npoint * nsample of a
 *      Conv2d block; n = b * p values per channel.  Any cin, cout, p >= 1; b <= 65535, p <= 65535 * PRCNN_TRAIN_CHUNK.
 *      No float atomics, no host read, no allocation: the caller sizes the workspaces with prcnn_train_layer_workspace.
 *
 * ARITHMETIC CONTRACT.  A cloud's positions are cut into consecutive chunks of PRCNN_TRAIN_CHUNK.  Every sum below has a shape that
 * is a function of (b, cin, cout, p) and the constants here alone, so the same input gives the same bits:
 *  (1) a product element -- z[i][co][q] = sum over ci of w[co][ci] x[i][ci][q], and dx[i][ci][q] = sum over co of w[co][ci] dz[i][co][q] --
 *      is the f32 fmaf chain over the summed index ASCENDING from +0.0f (what v_mfma_f32_32x32x2_f32 computes);
 *  (2) a per-channel sum over positions (of z and z * z in the forward; of g and g * zhat in the backward) is taken in f64: inside a
 *      chunk in a fixed tree -- forward: per column j of the chunk's 128-wide sub-tiles the terms at j, j + 128, ... left to right,
 *      the 32 columns of a quarter in the xor tree (distance 1, 2, 4, 8, 16), the four quarters left to right; backward: per
 *      thread t of 256 the terms at t, t + 256, ... left to right, the 64 lanes of a wave in the xor tree (1 .. 32), the four waves
 *      left to right -- then the chunks left to right from 0.0, cloud-major (cloud 0's chunks, cloud 1's, ...);
 *  (3) mean = S1 / n, var = max(S2 / n - mean * mean, 0), rstd = 1 / sqrt(var + eps) in f64 (stats (2,cout) f64: mean, rstd);
 *      running_mean = (1 - m) running_mean + m mean and running_var = (1 - m) running_var + m (var n / (n - 1)), f64, rounded once;
 *  (4) zhat = (z - mean) rstd, pre = zhat gamma + beta, y = max(pre, 0) per element in f64 from the f32 z, rounded once; without
 *      BatchNorm y = max(z + bias, 0) in f32 (one rounding); relu = 0 leaves the max out;
 *  (5) g = dy where pre > 0 (recomputed as in (4); without BatchNorm: where y > 0), else 0; dbeta (dbias) = s1 = sum g and
 *      dgamma = s2 = sum g zhat, rounded once; dz = gamma rstd ((g - s1 / n) - zhat (s2 / n)) per element in f64, rounded once;
 *      without BatchNorm dz = g;
 *  (6) dw[co][ci]: per (cloud, chunk) the f32 fmaf chain over the chunk's positions ascending of dz[i][co][q] x[i][ci][q] from
 *      +0.0f; these partials are added in f64 left to right, cloud-major, and rounded once. */
enum { PRCNN_TRAIN_CHUNK = 1024 };
/* element counts of the two workspaces: work (f64, *stat_f64 elements) and dw_work (f32, *dw_f32 elements; the backward's, needed
 * only where dw is wanted).  Contents arbitrary on entry. */
int prcnn_train_layer_workspace(int b, int cin, int cout, int p, long *stat_f64, long *dw_f32);
/* bn != 0: z, stats and y are written, running_mean / running_var (either may be NULL) updated in place; b * p = 1 is an error.
 * bn == 0: y = act(z + beta) with beta the bias (NULL: none); gamma, the running buffers, z, stats and work are not touched. */
int prcnn_train_layer_forward(int b, int cin, int cout, int p, int bn, int relu, const float *x, const float *w, const float *gamma,
                              const float *beta, double eps, double momentum, float *running_mean, float *running_var, float *z, float *y,
                              double *stats, double *work, void *stream);
/* zy is the saved z (bn != 0) or the saved y (bn == 0; read only with relu).  dz (b,cout,p) is scratch, written unless bn == 0 and
 * relu == 0.  dx, dw, dgamma, dbeta (the bias gradient when bn == 0) are each skipped when NULL. */
int prcnn_train_layer_backward(int b, int cin, int cout, int p, int bn, int relu, const float *dy, const float *x, const float *w,
                               const float *zy, const float *gamma, const float *beta, const double *stats, float *dz, float *dx, float *dw,
                               float *dgamma, float *dbeta, double *work, float *dw_work, void *stream);

/* ---- shared-MLP epilogues (fused forms of pytorch_utils.py Conv2d -> BN(eval) -> ReLU and of
 *      the max over nsample of pointnet2_modules.py:41-44; not in the reference ABI) ------------ */

/* x (outer, c, inner) f32 in place: x = max(x + bias[c], 0).  Replaces the separate bias-add and
 * ReLU passes after a bias-free 1x1 convolution (pytorch_utils.py:35-101). */
int prcnn_bias_relu_inplace(long outer, int c, long inner, const float *bias, float *x, void *stream);

/* in (b, c, npoint, nsample) = raw output of the LAST 1x1 convolution of a shared MLP ->
 * out (b, c, npoint) = relu(max_s in + bias[c]), which equals max_s relu(in + bias[c]) exactly
 * (F.max_pool2d over nsample, pointnet2_modules.py:41-44). */
int prcnn_maxpool_bias_relu(int b, int c, int npoint, int nsample, const float *bias,
                            const float *in, float *out, void *stream);

/* ---- point-major (channels-last) forms used by the MI355X inference path (csrc/pointmajor.hip);
 *      same values as K2 / the max-pool / K8, features stored (b, n, c) instead of (b, c, n) -------- */

/* Grouping for QueryAndGroup (pointnet2_utils.py:241-264) with point-major features (b,n,c):
 * out (b, m*nsample, kpad), kpad = round_up(c,4)+4, row = [features[idx] | 0-pad | xyz[idx]-centre | 0]. */
int prcnn_group_cat_pm(int b, int n, int m, int c, int nsample, const float *new_xyz, const float *xyz,
                       const float *features, const int *idx, float *out, void *stream);
/* First shared-MLP layer on grouped points without materialising the grouped input (the layer is
 * linear before its ReLU): P (b,n,cout) = features @ W1f^T + b1 per point, wxyz (3,cout) = the xyz
 * columns of W1 -> out (b, m*nsample, cout) = relu(P[idx] + wxyz . (xyz[idx] - new_xyz)). */
int prcnn_gather_affine_relu_pm(int b, int n, int m, int cout, int nsample, const float *new_xyz,
                                const float *xyz, const float *P, const float *wxyz, const int *idx,
                                float *out, void *stream);
/* One kernel for a set-abstraction MLP on grouped points (hand-written v_mfma_f32_32x32x2_f32 tiles):
 * gather -> layer 1 (P[idx] + wxyz.(xyz[idx]-centre), ReLU) -> layer 2 (w2t,b2,ReLU) -> layer 3
 * (w3t,b3,ReLU) -> max over nsample; nothing of the grouped activations touches HBM
 * (pointnet2_modules.py:37-53 for one scale).  w2t (c1,c2) / w3t (c2,c3) are stored input-channel-major.
 * Supported: c1 = c2 = 128, c3 in {128,256}, nsample = 64.  out[(b*m)][out_col..out_col+c3), row stride
 * out_stride. */
int prcnn_sa_mlp_fused(int b, int n, int m, int nsample, int c1, int c2, int c3, const float *new_xyz,
                       const float *xyz, const float *P, const float *wxyz, const int *idx, const float *w2t,
                       const float *b2, const float *w3t, const float *b3, float *out, int out_stride,
                       int out_col, void *stream);

/* The same fused set-abstraction MLP over the DISTINCT grouped rows only.  The reference's ball query back-fills the
 * slots beyond the hit count with the first hit (ball_query_gpu.cu:35-39) and the grouped MLP + max_pool2d
 * (pointnet2_utils.py:241-264, pointnet2_modules.py:37-53) evaluates those copies again; the max over a group does not
 * change when they are dropped.  prcnn_ball_pack: idx (b,m,nsample) -> per cloud, cnt[c] = 1 + (last slot that differs
 * from slot 0) rows per centre, written as a dense list of 64-row tiles:
 *   rowinfo  u32 [b * ceil(m*nsample/64) * 64]: (centre within cloud) << 16 | (point within cloud)
 *   rowdxyz  float4 [same length]: xyz[point] - new_xyz[centre] of the row (the grouped, centre-relative coordinates of
 *            pointnet2_utils.py:252), so that the MLP kernels do not gather coordinates again
 *   tilecloud i32 [b * ceil(m*nsample/64)]:     cloud of each tile
 *   hdr      u32 [4]: [0] tiles, [1] distinct rows (device-resident; no host sync)
 *   limit    i32 [b], optional: points k >= limit[cloud] of a cloud are copies of point k % limit[cloud] (the wrap-around
 *            fill of RoI pooling, roipool3d_kernel.cu:152-159); their rows are duplicates as well and are dropped
 * Every prcnn_ball_pack* entry takes m <= 15360 centres and n <= 65536 points per cloud (rowinfo keeps the point in 16 bits) and
 * refuses anything larger.
 * prcnn_sa_packed_mlp: layers as prcnn_sa_mlp_fused (c1 = c2 = 128; narrower levels zero-padded by the caller), c3 in
 * {128, 256}; zeroes out[(b*m)][out_col..out_col+c3) and accumulates the per-centre maxima with atomicMax (values are
 * >= 0 after ReLU).  Bit-identical to prcnn_sa_mlp_fused on the same idx.  max_tiles = b * ceil(m*nsample/64). */
int prcnn_ball_pack(int b, int n, int m, int nsample, const int *idx, const int *limit, const float *xyz,
                    const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr,
                    void *stream);
/* The same for b = lists x group clouds in one launch: list l = clouds [l group, (l+1) group) gets its own row list and header --
 * rowinfo / rowdxyz [lists][group * tiles_cap * 64], tilecloud [lists][group * tiles_cap] (cloud index INSIDE the list),
 * hdr [lists][4].  Used for the packed row lists of the batches of one geometry group (each batch's kernels walk their own tiles). */
int prcnn_ball_pack_groups(int b, int group, int n, int m, int nsample, const int *idx, const int *limit, const float *xyz,
                           const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr,
                           void *stream);

/* Every form of prcnn_ball_pack behind one entry (round 5): group = clouds per list (b: one list), limit / rep / crep optional (NULL),
 * hdr_is_zero != 0: hdr [lists][4] already holds zeros -- a slice of an arena the caller zeroes once per chain of launches instead of
 * one memset per row list. */
int prcnn_ball_pack_ex(int b, int group, int n, int m, int nsample, const int *idx, const int *limit, const int *rep, const int *crep,
                       const float *xyz, const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr,
                       int hdr_is_zero, void *stream);

/* prcnn_ball_pack with a representative map (round 3): rep (b,n) i32, rep[cloud][k] = the lowest-indexed point of the cloud
 * that is an exact copy of point k (coordinates and features; k when it is the first of its kind).  A copy lies in a ball
 * iff its representative does and the representative is listed earlier in the same row, so the slots whose point is not
 * its own representative are dropped from the row list as well (a max-pool over copies is the max-pool over the
 * originals: same bits as pointnet2_modules.py:37-53 over all nsample rows).  nsample <= 64 with rep.
 * crep (b,m) i32, optional: the same kind of map over the CENTRES (new_xyz): a centre that is an exact copy of an earlier
 * one gets no rows at all -- its pooled output is never computed (the caller's zero stays) and must not be read; the level
 * above passes this map as its `rep`, so it never is.  rep and crep may each be null. */
int prcnn_ball_pack_rep(int b, int n, int m, int nsample, const int *idx, const int *limit, const int *rep, const int *crep,
                        const float *xyz, const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud,
                        unsigned int *hdr, void *stream);

/* The representative map of the points an FPS call sampled: sel (b,m) i32 indexes clouds of n points of which the points
 * k >= limit[cloud] are copies of point k % limit[cloud] (RoI pooling's wrap-around fill, roipool3d_kernel.cu:152-159)
 * and / or prev (b,n) i32 is the representative map of those n points; rep (b,m) i32 <- the first sampled point with the
 * same source as sampled point j. */
int prcnn_dup_rep(int b, int n, int m, const int *sel, const int *limit, const int *prev, int *rep, void *stream);

/* The whole geometry chain of the RCNN's RoI clouds in ONE launch, a wave per RoI (csrc/roi_geometry.hip, round 3): xyz (b,512,3) pooled
 * coordinates whose points k >= limit[cloud] are copies of point k % limit[cloud] ->
 *   new_xyz1 (b,128,3), idx1 (b,128,ns1), rep1 (b,128)  = prcnn_fps_new_xyz(128), prcnn_ball_query_limit(r1, ns1), prcnn_dup_rep(limit)
 *   new_xyz2 (b,32,3),  idx2 (b,32,ns2),  rep2 (b,32)   = the same one level up over the 128 centres: prcnn_fps_new_xyz(32),
 *                                                         prcnn_ball_query(r2, ns2) into a zero-filled tensor, prcnn_dup_rep(prev = rep1)
 * -- rcnn_net.py:165-175 (SA modules 1 and 2 of the RCNN: pointnet2_modules.py:37-46 sampling + grouping indices) under
 * default.yaml's RCNN.NUM_POINTS 512, SA_CONFIG.NPOINTS [128, 32, -1].  n == 512, m1 == 128, m2 == 32, ns1, ns2 <= 64. */
int prcnn_rcnn_roi_geometry(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                            const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                            void *stream);
/* ... and the distinct-row lists of both levels out of the same launch (round 5; csrc/roi_geometry.hip roi_pack_out): what
 *   prcnn_ball_pack_ex(b, b, 512, 128, ns1, idx1, limit, NULL, rep1, xyz, new_xyz1, rowinfo1, rowdxyz1, tilecloud1, hdr1, ...) and
 *   prcnn_ball_pack_ex(b, b, 128, 32, ns2, idx2, NULL, rep1, rep2, new_xyz1, new_xyz2, rowinfo2, rowdxyz2, tilecloud2, hdr2, ...)
 * write -- every cloud's rows in the same order, cut into the same tiles; the order of the clouds' tiles inside a list is whatever
 * the list's counter hands out (as for prcnn_ball_pack).  Buffers sized as for prcnn_ball_pack: b * ceil(m * ns / 64) tiles per list;
 * hdr1 / hdr2 (4 u32 each) are zeroed by this call unless hdr_is_zero != 0 (the caller zeroed them: see prcnn_ball_pack_ex).
 * idx1 and idx2 may both be NULL: the index tensors are then not written (the packed MLP kernels read the row lists only).
 * tilecloud1 and tilecloud2 may both be NULL: the lists are then written in the form whose ROWS carry their cloud -- descriptor
 * (cloud << 16) | (centre << 9) | point, hdr[1] = rows, hdr[0] unused -- with every cloud's rows right behind another cloud's: tiles are
 * cut wherever the rows fall, no padded last tile per cloud.  prcnn_sa_packed_mlp takes such a list when IT is given tilecloud == NULL.
 * rowinfo3 / rowdxyz3 / hdr3 (all three or none; only with the row-carried form): the list of the GroupAll level above the two sampled ones
 * (rcnn_net.py:64-92, SA_CONFIG.NPOINTS[2] = -1: one group of all m2 centres, no centre subtraction) -- per cloud a row (centre 0, point j)
 * for every level-2 centre j that is its own representative, relative coordinates = new_xyz2[j]: what
 * prcnn_ball_pack_ex(b, b, m2, 1, m2, {0 .. m2-1}, NULL, rep2, NULL, new_xyz2, zeros, ...) lists; prcnn_sa_wide_fused3 reads it (tilecloud NULL).
 * crows1 / hdr_c1 (both or none): the level-1 centres that are their own representatives, as rows cloud * m1 + centre of a (b * m1)-row
 * matrix, hdr_c1[1] of them: the list prcnn_rows_gemm128_rows takes for level 2's per-point layer (the other centres copy an earlier one:
 * no row list names them, nobody reads their rows).
 * The reference has no counterpart: it groups all nsample rows (pointnet2_utils.py:241-264); see prcnn_ball_pack. */
int prcnn_rcnn_roi_geometry_packs(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                                  const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                                  unsigned int *rowinfo1, float *rowdxyz1, int *tilecloud1, unsigned int *hdr1,
                                  unsigned int *rowinfo2, float *rowdxyz2, int *tilecloud2, unsigned int *hdr2,
                                  unsigned int *rowinfo3, float *rowdxyz3, unsigned int *hdr3, int *crows1, unsigned int *hdr_c1,
                                  int hdr_is_zero, void *stream);
/* The "live rows" form of the same launch: of SA level 1 only what level 2 reads.  Level 2 is sampled and queried first; a level-1 centre
 * is LIVE iff a row of the level-2 list names it (37.6 of 49.9 distinct centres per RoI on the uniform synthetic scenes, 44.7 of 49.6 on
 * the LiDAR-shaped ones: profiles/r08_live_rows.md).  new_xyz*, rep*,
 * list 2 and list 3 are those of prcnn_rcnn_roi_geometry_packs; list 1 holds the live centres' rows only (each centre's rows as in the full
 * list, in centre order; with a tilecloud, a cloud's last tile is filled with copies of its last listed row), crows1 the live centres only.
 * used0 (b, 16) u32, every word written: bit k of a cloud's 512 = a row of its list 1 names pooled point k -- never empty (centre 0 is always
 * live and names point 0 at least); prcnn_pooled_rows_src_live takes it.  The index tensors are not written.  Nothing above level 2 reads a
 * centre that is not live and nothing reads a pooled point outside used0: the network's results are those of the full lists, bit for bit. */
int prcnn_rcnn_roi_geometry_live(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                                 const int *limit, float *new_xyz1, int *rep1, float *new_xyz2, int *rep2,
                                 unsigned int *rowinfo1, float *rowdxyz1, int *tilecloud1, unsigned int *hdr1,
                                 unsigned int *rowinfo2, float *rowdxyz2, int *tilecloud2, unsigned int *hdr2,
                                 unsigned int *rowinfo3, float *rowdxyz3, unsigned int *hdr3, int *crows1, unsigned int *hdr_c1,
                                 unsigned int *used0, int hdr_is_zero, void *stream);
/* out_is_zero (this entry, prcnn_sa_xyz_mlp_packed, prcnn_packed_layer_segmax): the results arrive through atomicMax into a
 * zeroed slice; 0 = the entry zeroes out[..., out_col : out_col + width) itself, 1 = the caller has zeroed it (one fill for all
 * the scales of a level instead of one strided fill per scale). */
/* tilecloud == NULL (this entry only, round 5): a list whose rows carry their cloud, as prcnn_rcnn_roi_geometry_packs writes it when it
 * is given no tilecloud either (n <= 512, m <= 128, b <= 65536): hdr[1] rows, tiles cut wherever they fall, the last tile's missing rows
 * read as copies of the list's last row.  Same per-row arithmetic: same bits as over the list with a tile per cloud. */
int prcnn_sa_packed_mlp(int b, int n, int m, int c3, long max_tiles, const float *P, const float *wxyz,
                        const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud,
                        const unsigned int *hdr, const float *w2t, const float *b2, const float *w3t,
                        const float *b3, float *out, int out_stride, int out_col, int out_is_zero, void *stream);

/* Shared-MLP layers of any width over packed row lists (csrc/packed_layer.hip): the levels whose weights do not fit the
 * register-resident fused kernels (RPN SA3/SA4: 128-196-256, 256-256-512, 256-384-512, pointrcnn/lib/config.py:58-61;
 * RCNN GroupAll level 256-256-512) run layer by layer on the distinct rows only.  Widths are zero-padded to multiples of
 * 128 by the caller; W is (K,N) input-channel-major; f32 MFMA, fixed summation order (oracle/mlp_oracle.c).
 *   prcnn_packed_gather_affine: A1 (max_tiles*64, c1) = relu(P[point] + wxyz.(xyz[point] - centre))   (layer 1)
 *   prcnn_packed_layer:         out[:, 0..n_store) = act(A @ W + bias)[:, 0..n_store) (n_store <= N: a head's narrow last layer,
 *                               weights zero-padded to N = 128) over hdr[0]*64 rows (hdr != NULL) or `rows` rows (hdr == NULL:
 *                               a plain row-major GEMM layer with a host-side row count, e.g. P = features @ W1f + b1)
 *   prcnn_packed_layer_segmax:  out[(b*m)][out_col..+N) = max over each centre's rows of relu(A @ W + bias)
 *                               (pointnet2_modules.py:37-53: last layer + max_pool2d) */
/* One scale of a wide set-abstraction level (layers 1-3 after the per-point part, max pool) over a packed row list in ONE
 * kernel (csrc/sa_wide.hip): what prcnn_packed_gather_affine + prcnn_packed_layer + prcnn_packed_layer_segmax compute, bit for
 * bit, without their activations going through HBM.  P (b,n,c1), wxyz (3,c1), w2 (c1,c2), w3 (c2,c3) k-major, widths multiples of
 * 128 as accepted by prcnn_sa_wide_fused_supported (RPN SA3 / SA4, RCNN GroupAll: pointrcnn/lib/config.py:58-61,118-120). */
int prcnn_sa_wide_fused_supported(int c1, int c2, int c3);
int prcnn_sa_wide_fused(int b, int n, int m, int c1, int c2, int c3, long max_tiles, const float *P, const float *wxyz,
                        const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud, const unsigned int *hdr,
                        const float *w2, const float *b2, const float *w3, const float *b3, float *out, int out_stride,
                        int out_col, int out_is_zero, void *stream);

/* The same scale with layer 1 inside as well (csrc/sa_wide3.hip): for a level that groups every point exactly once -- the RCNN's GroupAll
 * level, rcnn_net.py:64-92 with pointnet2_modules.py:19-55 -- the per-point part of layer 1 is the layer itself, and the separate
 * prcnn_packed_layer launch that made P (and P's trip through HBM) goes away.  F (b,n,c0) point features; wcat = w1 (c0,c1) | w2 (c1,c2) |
 * w3 (c2,c3), k-major, in ONE allocation; b1 / b2 / b3 the biases; the rest as prcnn_sa_wide_fused.  Results: prcnn_packed_layer (P = F w1 + b1)
 * followed by prcnn_sa_wide_fused, bit for bit. */
int prcnn_sa_wide_fused3_supported(int c0, int c1, int c2, int c3);
int prcnn_sa_wide_fused3(int b, int n, int m, int c0, int c1, int c2, int c3, long max_tiles, const float *F, const float *wxyz,
                         const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud, const unsigned int *hdr,
                         const float *wcat, const float *b1, const float *b2, const float *b3, float *out, int out_stride,
                         int out_col, int out_is_zero, void *stream);

/* Batched forms: up to 4 independent problems (the scales of one MSG level, pointnet2_modules.py:19-55 loops over them) in ONE
 * launch -- the sparse levels are latency-bound, side by side they cost one launch instead of one each.  The single-problem
 * entries below are these with n = 1.  segmax = 1: every problem is a level's last layer + max pool (fields b, m, rowinfo,
 * tilecloud, out_col, out_is_zero; ldo = row stride of the level's output); segmax = 0: plain layers (fields rows, n_store,
 * relu; hdr NULL = host row count). */
typedef struct prcnn_gather_problem {
    int b, n, c1; long max_tiles; const float *P; const float *wxyz; const unsigned int *rowinfo; const float *rowdxyz;
    const int *tilecloud; const unsigned int *hdr; float *out;
} prcnn_gather_problem;
typedef struct prcnn_layer_problem {
    const unsigned int *hdr; long rows; long max_tiles; int K, N, n_store; const float *A; long lda; const float *W;
    const float *bias; int relu; float *out; long ldo;
    int b, m; const unsigned int *rowinfo; const int *tilecloud; int out_col, out_is_zero;
} prcnn_layer_problem;
/* one 128-wide problem of prcnn_sa_packed_mlp (c3 = 128): the two scales of an MSG level go into ONE launch (round 5) */
typedef struct prcnn_sa_problem {
    int b, n, m, c3; long max_tiles; const float *P; const float *wxyz; const unsigned int *rowinfo; const float *rowdxyz;
    const int *tilecloud; const unsigned int *hdr; const float *w2t; const float *b2; const float *w3t; const float *b3;
    float *out; int out_stride, out_col, out_is_zero;
    int c1, c2;     /* the REAL widths of layers 1 and 2 when the 128-wide arrays are zero-padded (0 = 128): 64-64 and 64-96, the scales of
                     * RPN SA2 (tools/cfgs/default.yaml SA_CONFIG.MLPS[1]), skip the padding's MFMAs -- same bits as the padded chain */
} prcnn_sa_problem;
int prcnn_sa_packed_mlp_batch(int nprob, const prcnn_sa_problem *problems, void *stream);
int prcnn_packed_gather_affine_batch(int nprob, const prcnn_gather_problem *problems, void *stream);
int prcnn_packed_layer_batch(int nprob, const prcnn_layer_problem *problems, int segmax, void *stream);
int prcnn_packed_gather_affine(int b, int n, int c1, long max_tiles, const float *P, const float *wxyz,
                               const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud,
                               const unsigned int *hdr, float *out, void *stream);
int prcnn_packed_layer(const unsigned int *hdr, long rows, long max_tiles, int K, int N, int n_store, const float *A,
                       long lda, const float *W, const float *bias, int relu, float *out, long ldo, void *stream);
/* EXPERIMENT (round 6, numerics switch PRCNN_SPLIT_BF16, default off; csrc/split_bf16.hip): the plain per-point layer of prcnn_packed_layer
 * (hdr == NULL form) on the bf16 matrix cores, every operand split exactly into three bf16 pieces, six products per k-step of 16,
 * f32 accumulation: ~1e-7 relative to the f32 fma chain, not its bits.  prcnn_split_weights_bf16x3: W (K, N) f32 -> `out`
 * ((K / 16) * (N / 32) * 3 * 64 * 16 bytes: the B operands of v_mfma_f32_32x32x16_bf16 in issue order), once per weight matrix;
 * prcnn_rows_layer_bf16x3: out[:, 0..n_store) = act(A @ W + bias).  K % 16 == 0, N % 128 == 0, lda % 4 == 0, A 16-byte aligned.
 * Replaces nothing of the reference's (its convolutions are a GEMM library's: pytorch_utils.py:35-101); measured in profiles/r06_split_bf16.md. */
int prcnn_split_weights_bf16x3(int K, int N, const float *W, void *out, void *stream);
int prcnn_rows_layer_bf16x3(long rows, int K, int N, int n_store, const float *A, long lda, const void *wsplit, const float *bias,
                            int relu, float *out, long ldo, void *stream);
/* First layer of a feature-propagation module (pointnet2_modules.py:139-156) with the interpolation moved behind the layer's
 * linear part: out[r] = act((A[r] @ W + bias) + ((w0 G[i0] + w1 G[i1]) + w2 G[i2])), A (rows,K) = the skip features, W (K,N) = the
 * skip columns of the layer, G = coarse features @ the interpolated columns of the layer (clouds * m_known rows, N wide),
 * idx / weight (rows,3) from prcnn_three_nn, row r in cloud r / n_per_cloud.  K, N multiples of 128. */
int prcnn_packed_layer_interp(long rows, int K, int N, const float *A, long lda, const float *W, const float *bias, int relu,
                              float *out, long ldo, int n_per_cloud, int m_known, const float *G, long ldg, const int *idx,
                              const float *weight, void *stream);
/* out[r][0..n) = A[r] @ W + bias for n <= 4 outputs (the 1-wide last layer of the classification heads, rpn.py:36-50,
 * rcnn_net.py:94-103): W (K,n) k-major; 32 lanes per row, fixed summation order (oracle: orc_rows_dot). */
/* The coordinates-only first SA level (prcnn_sa_xyz_mlp) over a packed row list: distinct rows only, bit-identical. */
int prcnn_sa_xyz_mlp_packed(int b, int m, int c1, int c2, int c3, long max_tiles, const unsigned int *rowinfo,
                            const float *rowdxyz, const int *tilecloud, const unsigned int *hdr, const float *w1,
                            const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                            float *out, int out_stride, int out_col, int out_is_zero, void *stream);
int prcnn_rows_dot(long rows, int K, int n, const float *A, long lda, const float *W, const float *bias, float *out,
                   long ldo, void *stream);
/* The last stretch of the RPN over all input points in one kernel (csrc/rpn_tail.hip): three_interpolate of the coarse
 * features (pointnet2_modules.py:136-160, FP module 0, no skip features) -> SharedMLP 256-128-128 -> the backbone features,
 * and on them the cls head 128-128-1 and the reg head 128-128-n_reg (rpn.py:28-50).  known (b,m,256), idx / weight (b,n,3)
 * from three_nn; wcat (768,128) = [FP layer 1 (256 rows) | FP layer 2 | cls layer 1 | reg layer 1 | reg layer 2 zero-padded
 * beyond n_reg columns], bcat (5,128) their biases, wc2 (128) / bc2 (1) the score layer; BN folded, k-major.
 * feats (b*n,128), cls (b*n), reg (b*n,n_reg), n_reg % 4 == 0.  Same arithmetic as prcnn_three_interpolate_pm ->
 * prcnn_packed_layer x5 -> prcnn_rows_dot, bit for bit. */
int prcnn_rpn_tail(int b, int n, int m, const float *known, const int *idx, const float *weight, const float *wcat,
                   const float *bcat, const float *wc2, const float *bc2, int n_reg, float *feats, float *cls, float *reg,
                   void *stream);
/* prcnn_rpn_tail with the FP module's first layer applied at the COARSE level (round 3): relu(W1 interp(f) + b1) =
 * relu(interp(W1 f) + b1).  G (b,m,128) = f @ W1 (no bias; prcnn_packed_layer over the 4096 coarse points of a scene, a
 * quarter of the rows); wcat (512,128) = [FP layer 2 | cls layer 1 | reg layer 1 | reg layer 2 zero-padded beyond n_reg
 * columns], bcat (5,128) = the biases of FP layer 1 (added after the interpolation), FP layer 2, cls 1, reg 1, reg 2.
 * Another association of the same sums than pointnet2_modules.py:139-156 (~1e-7 relative). */
int prcnn_rpn_tail_lin(int b, int n, int m, const float *G, const int *idx, const float *weight, const float *wcat,
                       const float *bcat, const float *wc2, const float *bc2, int n_reg, float *feats, float *cls,
                       float *reg, void *stream);
/* prcnn_rpn_tail_lin with the proposal layer's decode INSIDE (round 5): boxes (b*n,7) = decode_bbox_target(xyz, reg, anchor,
 * get_xz_fine = True, get_y_by_bin = False, get_ry_fine = False) with y += h / 2 (lib/utils/bbox_transform.py:24-121,
 * lib/rpn/proposal_layer.py:23-31), operation for operation what prcnn_rpn_proposals' decode computes from the stored rows; the
 * (b*n, n_reg) regression rows themselves never reach HBM.  Served regression layout: prcnn_rpn_tail_boxes_supported (12 x / z bins,
 * 12 heading bins, fine residuals: the 76 channels of every shipped yaml); anchor_size_host: (h, w, l) in HOST memory; xyz (b,n,3). */
int prcnn_rpn_tail_boxes_supported(int channels, float loc_scope, float loc_bin_size, int num_head_bin, int xz_fine);
/* test hook of that decode's branch-free f32 fmod by 2 pi: out_mine[i] = its value, out_lib[i] = fmodf(a[i], (float)(2 pi)) */
int prcnn_selftest_fmod_two_pi(long n, const float *a, float *out_mine, float *out_lib, void *stream);
int prcnn_rpn_tail_lin_boxes(int b, int n, int m, const float *G, const int *idx, const float *weight, const float *wcat,
                             const float *bcat, const float *wc2, const float *bc2, int n_reg, float loc_scope, float loc_bin_size,
                             int num_head_bin, int xz_fine, const float *anchor_size_host, const float *xyz, float *feats,
                             float *cls, float *boxes, void *stream);
int prcnn_packed_layer_segmax(int b, int m, long max_tiles, int K, int N, const float *A, long lda, const float *W,
                              const float *bias, const unsigned int *rowinfo, const int *tilecloud,
                              const unsigned int *hdr, float *out, int out_stride, int out_col, int out_is_zero, void *stream);

/* Entrance of the RCNN as MFMA kernels (lib/net/rcnn_net.py:139-163 xyz_up_layer + concat + merge_down_layer,
 * fused with the per-point part of SA1's first layer): rows (r, ld) f32 = pooled rows
 * [x',y',z',mask,depth,0,0,0 | 128 RPN features at column fcol] as prcnn_roipool3d_canonical writes them, r % 64 == 0;
 * wu1 (8,128), wu2 (128,128), wm (256,128), wp (128,128) k-major with BN folded;
 * xfeat (r,128) = xyz_up output, merged (r,128) = relu([xfeat | feats] wm + bm), p (r,128) = merged wp + bp:
 * three launches of one tiled MFMA layer kernel, all buffers caller-allocated.
 * tilemap / ntiles (optional, both or neither): only the 64-row tiles listed in tilemap[0 .. *ntiles) are computed -- the
 * tiles that hold DISTINCT pooled rows (prcnn_pooled_tiles from prcnn_roipool3d_canonical's pooled_cnt); the rows of the
 * other tiles are wrap-around copies (roipool3d_kernel.cu:152-159) that no consumer reads, and are left unwritten. */
int prcnn_rcnn_point_mlp(long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1,
                         const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                         const float *bp, float *xfeat, float *merged, float *p, const int *tilemap,
                         const unsigned int *ntiles, void *stream);
int prcnn_pooled_tiles(int clouds, int rows_per_cloud, const int *cnt, int *tilemap, unsigned int *hdr, void *stream);
/* The same chain (only p) over a LIST of rows instead of whole tiles (round 5): prcnn_pooled_rows lists the distinct pooled rows of all
 * clouds back to back -- rowmap[0 .. hdr[1]), row c * rows_per_cloud + j for j < max(cnt[c], 1), the clouds in the order a device counter
 * hands out; hdr (4 u32) is zeroed by the call unless hdr_is_zero -- and prcnn_rcnn_point_mlp_rows computes p for exactly those rows,
 * 64 list entries per tile whichever RoIs they belong to (a RoI's 47 distinct rows no longer fill a tile of 64).  p rows that are not
 * listed are left as they are.  Per row the arithmetic is prcnn_rcnn_point_mlp's: same bits. */
int prcnn_pooled_rows(int clouds, int rows_per_cloud, const int *cnt, int *rowmap, unsigned int *hdr, int hdr_is_zero, void *stream);
int prcnn_rcnn_point_mlp_rows(long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1,
                              const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                              const float *bp, float *p, const int *rowmap, const unsigned int *hdr, void *stream);
/* The list and the chain over pooled rows that carry NO features (prcnn_roipool3d_canonical_src: rows of 8 floats and src, each row's
 * row of the RPN's (points, 128) feature matrix).  prcnn_pooled_rows_src = prcnn_pooled_rows that also writes featmap[e] = src[rowmap[e]]
 * in the same pass (src, featmap: both or neither; src (clouds * rows_per_cloud) i32).  prcnn_rcnn_point_mlp_rows_src: rows (r, ld >= 8)
 * [x',y',z',mask,depth, ...]; list entry e takes its 128 features from row featmap[e] of feats, zeros where featmap[e] < 0 (the one listed
 * row of an empty box).  Nothing is copied between the RPN's feature matrix and the chain; per row the arithmetic is
 * prcnn_rcnn_point_mlp's: same bits. */
int prcnn_pooled_rows_src(int clouds, int rows_per_cloud, const int *cnt, const int *src, int *rowmap, int *featmap, unsigned int *hdr,
                          int hdr_is_zero, void *stream);
/* ... over the rows that a set names: used (clouds * ceil(rows_per_cloud / 32)) u32, bit j of a cloud's words = row j of it is read
 * (prcnn_rcnn_roi_geometry_live's used0) -> rows j < max(cnt[c], 1) with their bit set, in row order per cloud; same header, same counter. */
int prcnn_pooled_rows_src_live(int clouds, int rows_per_cloud, const int *cnt, const unsigned int *used, const int *src, int *rowmap,
                               int *featmap, unsigned int *hdr, int hdr_is_zero, void *stream);
int prcnn_rcnn_point_mlp_rows_src(long r, int ld, const float *rows, const float *feats, const float *wu1, const float *bu1,
                                  const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                                  const float *bp, float *p, const int *rowmap, const int *featmap, const unsigned int *hdr,
                                  void *stream);

/* One 128-wide shared-MLP / Conv1d layer (pytorch_utils.py:35-101 with BN folded) on the same tiled MFMA kernel:
 * out (r,128) = act(A0 w[0:128] [+ A1 w[128:256]] + bias), r % 64 == 0; A0 = src0 rows (128 floats at column col0, row
 * stride ld0), npanel = 2 adds A1 = src1 rows (col1, ld1): a K = 256 layer over two 128-wide halves. w k-major. */
/* the same 128 -> 128 layer (npanel = 1) over a LIST of rows: out[r] = act(src[r] @ w + bias) for r = rowmap[0 .. hdr[1]), rows that are not
 * listed are neither read nor written (round 5; per row the arithmetic of prcnn_rows_gemm128 / prcnn_packed_layer: same bits) */
int prcnn_rows_gemm128_rows(long r, const float *src, int ld, int col, const float *w, const float *bias, int relu, float *out,
                            const int *rowmap, const unsigned int *hdr, void *stream);
int prcnn_rows_gemm128(long r, int npanel, const float *src0, int ld0, int col0, const float *src1, int ld1, int col1,
                       const float *w, const float *bias, int relu, float *out, void *stream);

/* One whole coordinates-only set-abstraction scale (first RPN SA level: QueryAndGroup without input features ->
 * 3-layer shared MLP + ReLU -> max over nsample; pointnet2_modules.py:37-53, pointnet2_utils.py:241-264) in one
 * VALU kernel: a grouped row lives in one lane from the gather to the max, weights are scalar operands.
 * xyz (b,n,3), new_xyz (b,m,3), idx (b,m,nsample); w1 (>=3,c1), w2 (c1,c2), w3 (c2,c3) k-major, BN folded;
 * out[(b*m rows)][out_col .. out_col+c3), row stride out_stride.
 * Supported (c1,c2,c3,nsample): (16,16,32,16), (32,32,64,32) -- prcnn_sa_xyz_mlp_supported returns 1 for those. */
int prcnn_sa_xyz_mlp_supported(int c1, int c2, int c3, int nsample);
int prcnn_sa_xyz_mlp(int b, int n, int m, int nsample, int c1, int c2, int c3, const float *new_xyz,
                     const float *xyz, const int *idx, const float *w1, const float *b1, const float *w2,
                     const float *b2, const float *w3, const float *b3, float *out, int out_stride, int out_col,
                     void *stream);
/* max over ns consecutive rows: in (rows_out*ns, c) -> out[r][out_col..out_col+c), row stride out_stride
 * (F.max_pool2d over nsample, pointnet2_modules.py:41-44, on the point-major MLP output). */
int prcnn_maxpool_pm(long rows_out, int ns, int c, const float *in, float *out, int out_stride,
                     int out_col, void *stream);
/* three_interpolate (interpolate_gpu.cu:77-97) on point-major features (b,m,c); result written into a
 * column slice of out (b, n, out_stride). */
int prcnn_three_interpolate_pm(int b, int c, int m, int n, const float *features, const int *idx,
                               const float *weight, float *out, int out_stride, int out_col, void *stream);
/* The input of a feature-propagation module in one pass (pointnet2_modules.py:139-151: three_interpolate, then torch.cat with
 * the skip features): out (b, n, c + c_skip) = [interpolated (same arithmetic as above) | skip (b, n, c_skip)];
 * c, c_skip multiples of 4, pointers 16-byte aligned. */
int prcnn_three_interpolate_cat_pm(int b, int c, int m, int n, const float *features, const int *idx, const float *weight,
                                   const float *skip, int c_skip, float *out, void *stream);

/* ---- iou3d_cuda ---------------------------------------------------------------------- */

/* boxes_overlap_bev_gpu  src/iou3d.cpp:31-50 -> src/iou3d_kernel.cu:223-234.
 * boxes_a (na,5), boxes_b (nb,5) [x1,y1,x2,y2,ry] -> ans (na,nb) intersection area. */
int prcnn_boxes_overlap_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                            float *ans_overlap, void *stream);
/* boxes_iou_bev_gpu  src/iou3d.cpp:52-71 -> src/iou3d_kernel.cu:236-248. */
int prcnn_boxes_iou_bev(int num_a, const float *boxes_a, int num_b, const float *boxes_b,
                        float *ans_iou, void *stream);
/* nms_gpu  src/iou3d.cpp:73-120 -> src/iou3d_kernel.cu:250-292 + host reduce.
 * boxes (n,5) DEVICE, score-sorted; keep (n) HOST int64.  BLOCKING (as the reference's
 * cudaMemcpy is).  Returns num_to_keep >= 0, or a negative PRCNN_E* code. */
int prcnn_nms(int boxes_num, const float *boxes, long long *keep_host, float thresh, void *stream);
/* nms_normal_gpu  src/iou3d.cpp:123-170 -> src/iou3d_kernel.cu:306-348. */
int prcnn_nms_normal(int boxes_num, const float *boxes, long long *keep_host, float thresh, void *stream);

/* Device-resident, batched greedy NMS (no host round trip): `nprob` independent problems.
 * boxes (nprob, n_max, 5) score-sorted per problem; counts (nprob) DEVICE i32 = valid rows of
 * each problem (NULL -> all n_max).  Writes keep (nprob, max_keep) i32 (row indices, padded
 * with -1) and num_keep (nprob) i32 = min(#kept, max_keep): exactly the first max_keep
 * entries the reference's full greedy pass would return.  rotated != 0 -> iou_bev, else
 * iou_normal.  Asynchronous. */
int prcnn_nms_device(int nprob, int n_max, const int *counts, const float *boxes, float thresh,
                     int rotated, int max_keep, int *keep, int *num_keep, void *stream);

/* The per-point RCNN inputs of point_rcnn.py:44-52 and rcnn_net.py:131-137 in one launch: seg[r] = sigmoid(scores[r]) > thresh ? 1 : 0,
 * depth[r] = |xyz[r]|, depth_norm[r] = depth[r] / 70 - 0.5  (rows = b * n; the reference's Python: sigmoid, compare, cast, norm, divide,
 * subtract -- six launches). */
int prcnn_point_aux(long rows, float thresh, const float *scores, const float *xyz, float *seg, float *depth, float *depth_norm,
                    void *stream);

/* Whole RPN proposal layer (lib/rpn/proposal_layer.py:15-119 + decode_bbox_target of
 * lib/utils/bbox_transform.py:24-121, distance-based variant) in five launches and no host sync:
 * decode -> per-scene score sort -> (0,40] / (40,80] m band selection (top 70 % / 30 % of pre_nms_top_n,
 * with the "no far points" fallback) -> batched NMS -> rois (b, post_nms_top_n, 7) + raw scores, zero padded.
 * xyz (b,n,3), scores (b,n), reg (b,n,channels); anchor_size_host = 3 floats in HOST memory (h,w,l).
 * n <= 65536 per scene (round 5: the chunked sort and the band scan take any n; tools/cfgs/double.yaml has 32768).
 * Quotas: post_nms_top_n <= 512 (near int(0.7 post) <= 358, far post - near <= 154), near >= far for both pre and post; anything
 * else returns PRCNN_EINVAL "rpn_proposals: unsupported quotas".  post <= 128 (inference) and 129..512 (TRAIN.RPN_POST_NMS_TOP_N)
 * differ in the axis-aligned NMS's kept-box table (256 / 512 rows of LDS) and in the trips of the assembly, not in any decision. */
int prcnn_rpn_proposals(int b, int n, int channels, float loc_scope, float loc_bin_size, int num_head_bin,
                        int xz_fine, const float *anchor_size_host, int pre_nms_top_n, int post_nms_top_n,
                        float nms_thresh, int rotated_nms, const float *xyz, const float *scores,
                        const float *reg, float *rois, float *roi_scores, void *stream);
/* The same layer over boxes decoded already (prcnn_rpn_tail_lin_boxes): boxes (b,n,7), scores (b,n). */
int prcnn_rpn_proposals_boxes(int b, int n, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated_nms,
                              const float *scores, const float *boxes, float *rois, float *roi_scores, void *stream);

/* Final detection stage of eval_rcnn.py (tools/eval_rcnn.py:506-530 decode with get_xz_fine = get_ry_fine
 * = True, :611-629 score threshold + rotated NMS) in three launches and no host sync.
 * rois (b,m,7), rcnn_reg (b,m,channels), rcnn_cls (b,m) raw scores, m <= 128.
 * pred_boxes3d (b,m,7) = every RoI's decoded box (RoI order); boxes (b,m,7) / scores (b,m) raw = survivors of
 * sigmoid(score) > score_thresh and rotated NMS, descending score, zero padded; num (b) i32. */
int prcnn_rcnn_postprocess(int b, int m, int channels, float loc_scope, float loc_bin_size, int num_head_bin,
                           int y_by_bin, float loc_y_scope, float loc_y_bin_size, const float *anchor_size_host,
                           float score_thresh, float nms_thresh, const float *rois, const float *rcnn_reg,
                           const float *rcnn_cls, float *pred_boxes3d, float *boxes, float *scores, int *num,
                           void *stream);
/* The same with the results as one BLOB per batch of scenes_per_blob scenes (b a multiple of it): blobs (b / spb, spb (8 m + 1)) f32,
 * each [spb m 7 boxes | spb m scores | spb num as i32 bits]: a launch over several batches hands every batch's detections to the
 * host with one copy (round 5). */
int prcnn_rcnn_postprocess_blobs(int b, int m, int channels, float loc_scope, float loc_bin_size, int num_head_bin,
                                 int y_by_bin, float loc_y_scope, float loc_y_bin_size, const float *anchor_size_host,
                                 float score_thresh, float nms_thresh, const float *rois, const float *rcnn_reg,
                                 const float *rcnn_cls, float *pred_boxes3d, float *blobs, int scenes_per_blob, void *stream);

/* ---- roipool3d_cuda ------------------------------------------------------------------ */

/* forward  src/roipool3d.cpp:48-79 -> roipool3dLauncher src/roipool3d_kernel.cu:209-237.
 * xyz (B,N,3), boxes3d (B,M,7) already enlarged, pts_feature (B,N,C) ->
 * pooled_features (B,M,S,3+C) and pooled_empty_flag (B,M), both zero-filled by the caller;
 * rows of empty boxes are left untouched. */
int prcnn_roipool3d(int batch_size, int pts_num, int boxes_num, int feature_in_len,
                    int sampled_pts_num, const float *xyz, const float *boxes3d,
                    const float *pts_feature, float *pooled_features, int *pooled_empty_flag,
                    void *stream);

/* RCNN input assembly in one pass (lib/net/rcnn_net.py:139-163 + roipool3d_utils.py:7-28 + kitti_utils.py:150-160):
 * enlarge the RoIs by pool_extra_width, pool the first `sampled` points per box (same selection as prcnn_roipool3d),
 * move the pooled coordinates into the RoI's canonical frame and write rows
 * [x', y', z', seg mask, depth, 0, 0, 0 | c features] (c % 4 == 0).  rois (b,m,7) are the UN-enlarged proposals;
 * feats (b,n,c) point-major; seg_mask, depth (b,n); pooled (b,m,sampled,8+c) need not be cleared; empty (b,m) i32.
 * pooled_cnt (b,m) i32, optional (NULL = off): number of DISTINCT rows of each box (min(#points in box, sampled), >= 1;
 * rows s >= cnt are the wrap-around copies of row s % cnt, roipool3d_kernel.cu:152-159).  When given, the feature
 * columns are written only for rows < round_up(cnt, 64): the coordinate / mask / depth columns of all rows are. */
/* pxyz / aabb (optional, both or neither): the cloud's spatial groups from prcnn_point_groups -- the selection then tests
 * pts_num / 64 group boxes and reads the few groups that can hold a point of the box instead of sweeping all points; same
 * points, same order (the hits are sorted by original index).  pts_num % 64 == 0, <= 65536. */
int prcnn_roipool3d_canonical(int batch_size, int pts_num, int boxes_num, int feature_len, int sampled_pts_num,
                              float pool_extra_width, const float *xyz, const float *rois, const float *feats,
                              const float *seg_mask, const float *depth, float *pooled, int *pooled_empty_flag,
                              int *pooled_cnt, const float *pxyz, const float *aabb, void *stream);
/* the same with xyz_out (b,m,sampled,3), optional (NULL = off): the rows' canonical coordinates once more as dense clouds -- what the
 * RCNN stage's sampling and ball queries (rcnn_net.py:165-175: pointnet2 SA modules over xyz = pooled[..., 0:3]) read. */
int prcnn_roipool3d_canonical_xyz(int batch_size, int pts_num, int boxes_num, int feature_len, int sampled_pts_num,
                                  float pool_extra_width, const float *xyz, const float *rois, const float *feats,
                                  const float *seg_mask, const float *depth, float *pooled, int *pooled_empty_flag,
                                  int *pooled_cnt, const float *pxyz, const float *aabb, float *xyz_out, void *stream);
/* The form that copies no features: the same selection, rows (b,m,sampled,8) = [x', y', z', seg mask, depth, 0, 0, 0] of ALL rows, and
 * src (b,m,sampled) i32 = the row of the (b * pts_num, c) feature matrix that each pooled row stands for: b * pts_num + point for the
 * distinct rows, the value of row s % cnt for the wrap-around rows, -1 in every slot of an empty box (whose features are zero rows).
 * pooled_cnt, pooled_empty_flag, pxyz / aabb, xyz_out as above.  The reader gathers at the source (prcnn_rcnn_point_mlp_rows_src). */
int prcnn_roipool3d_canonical_src(int batch_size, int pts_num, int boxes_num, int sampled_pts_num, float pool_extra_width,
                                  const float *xyz, const float *rois, const float *seg_mask, const float *depth, float *rows,
                                  int *src, int *pooled_empty_flag, int *pooled_cnt, const float *pxyz, const float *aabb,
                                  float *xyz_out, void *stream);
/* Spatial groups of clouds xyz (b,n,3), n % 64 == 0, n <= 65536: pxyz (b,n,4) = the points in Morton order over (x,z) with the
 * original index in the 4th lane (int bits), aabb (b, n/64, 2, 4) = min / max corner of every 64-point group.  Any box-vs-cloud
 * sweep (RoI pooling here) can cull by group.  Not part of the reference ABI. */
int prcnn_point_groups(int b, int n, const float *xyz, float *pxyz, float *aabb, void *stream);

/* The reference module's two HOST utilities (CPU tensors, unbatched; they serve its dataset / GT-database code):
 * pts_in_boxes3d_cpu  roipool3d.cpp:97-125 -> flags (boxes_num, pts_num) i64 in {0,1};
 * roipool3d_cpu       roipool3d.cpp:127-195 -> pooled_pts (boxes_num,sampled,3), pooled_features
 * (boxes_num,sampled,feature_len), empty (boxes_num) i64; rows of empty boxes stay as the caller left them.
 * HOST pointers, no stream. */
int prcnn_host_pts_in_boxes3d(int boxes_num, int pts_num, const float *pts, const float *boxes3d, long long *flags);
int prcnn_host_roipool3d(int boxes_num, int pts_num, int feature_len, int sampled, const float *pts,
                         const float *boxes3d, const float *pts_feature, float *pooled_pts, float *pooled_features,
                         long long *empty);

/* ---- evaluate/rotate_iou.py ---------------------------------------------------------- */

/* rotate_iou_gpu_eval  evaluate/rotate_iou.py:294-329 (kernel :261-291).
 * boxes (n,5), query_boxes (k,5) [cx,cy,w,h,angle] DEVICE -> iou (n,k);
 * criterion -1 IoU, 0 /area(query), 1 /area(box), 2 raw intersection (as the kernel passes
 * (query, box) to the device function, :287-291). */
int prcnn_rotate_iou_eval(int n, int k, const float *boxes, const float *query_boxes,
                          float *iou, int criterion, void *stream);

/* Block-diagonal rotate_iou_gpu_eval: segment s (one image) pairs boxes[box_off[s]..box_off[s+1]) with
 * query_boxes[q_off[s]..q_off[s+1]) and writes its row-major block at out_off[s]; one launch for a whole split
 * instead of the ~50 dense parts of evaluate/eval2.py:352-424 (calculate_iou_partly), whose cross-image pairs
 * are discarded.  out_off (nseg+1) i64, box_off / q_off (nseg+1) i32, all DEVICE; total = out_off[nseg]. */
int prcnn_rotate_iou_eval_segmented(int nseg, long long total, const long long *out_off, const int *box_off,
                                    const int *q_off, const float *boxes, const float *query_boxes, float *iou,
                                    int criterion, void *stream);

/* Fused best match over the segmented layout above (csrc/eval_match.hip; evaluate/evaluate.py:135-207 takes np.max / np.argmax of
 * every image's BEV overlap block, along both axes).  n = box_off[nseg] boxes, k = q_off[nseg] queries, offsets DEVICE i32.
 * -> row_val (n) f32 / row_idx (n) i32: for every box the maximum over its segment's queries of the pair value
 * prcnn_rotate_iou_eval_segmented would have written (bit-equal) and the segment-local index where it is first reached;
 * col_val (k) / col_idx (k): the same for every query over its segment's boxes, both may be NULL.  A segment whose other side is
 * empty yields value 0 and index -1.  No (n x k) buffer exists anywhere. */
int prcnn_bev_best_match(int nseg, int n, int k, const int *box_off, const int *q_off, const float *boxes,
                         const float *query_boxes, int criterion, float *row_val, int *row_idx, float *col_val, int *col_idx,
                         void *stream);

/* align_size (mode 0) / align_front (mode 1) of evaluate/evaluate.py:187-230, one thread per detection, f64, DEVICE pointers.
 * location (n,3) and dimensions (n,3; stored l, h, w) are rewritten in place for detections whose row_val, widened to f64, is
 * > 0.2: dimensions take the matched ground-truth row of gt_dimensions (q_off[segment] + row_idx), align_front first shifts the
 * location along the box axes by half the size differences.  branch (n) i32 or NULL: -1 untouched, else bit 0 first shift taken,
 * bit 1 its 0 < alpha choice, bit 2 second shift taken, bit 3 its |alpha| < pi / 2 choice. */
int prcnn_eval_align(int nseg, int n, const int *box_off, const int *q_off, double *location, double *dimensions,
                     const double *alpha, const double *rotation_y, const double *gt_dimensions, const float *row_val,
                     const int *row_idx, int mode, int *branch, void *stream);

/* ---- lib/datasets/kitti_rcnn_dataset.py: the network-input stage on the device ---------- */

/* get_lidar + get_valid_flag + the near/far sampler of get_rpn_sample (kitti_rcnn_dataset.py:249-324) with
 * calibration.py:51-71, one workgroup per scene.  raw (b,n_max,stride) f32, stride 3 or 4, as read from velodyne .bin
 * (lidar_frame = 1) or already rectified (0); counts (b) i32; calib (b,PRCNN_CALIB_ROW) f32 = V2C 3x4 | R0 3x3 | P2 3x4 | img h, w;
 * image_filter 0/1 (in-image + depth >= 0 test); scope_host = 6 HOST doubles x0,x1,y0,y1,z0,z1 (the f64 PC_AREA_SCOPE: the f32
 * coordinates are compared with it in double, as kitti_io.valid_flag does; read before the call returns) or NULL;
 * seeds (b) u64 DEVICE.  -> out (b,npoints,3), stats (b,3) i32 = #valid, #near, #far, choice (b,npoints) i32 = raw
 * index of each output point (may be NULL).  npoints <= 16384.
 * The subset is random (distinct-key selection + key-sorted shuffle): same distribution as the reference's
 * np.random.choice / shuffle, not the same draws; transform and filter are bitwise the reference's (see prcnn_valid_flags).
 * Given the class of every raw point and the seed, every output row is determined: tests/input_stage_ref.py is the definition,
 * and the kernel equals it pick for pick.  A scene in which nothing is taken -- no valid point, or npoints_faraway = 0 with more
 * than npoints valid points that are all far -- is an empty scene: out zeros, choice -1, stats as counted. */
enum { PRCNN_CALIB_ROW = 35 };   /* floats per calibration row, here and in every batch struct below whose `calib` has this layout */
int prcnn_input_stage(int b, int n_max, int stride, int lidar_frame, int image_filter, const int *counts,
                      const float *raw, const float *calib, const double *scope_host, int npoints, float far_depth,
                      int npoints_faraway, const unsigned long long *seeds, float *out, int *stats, int *choice,
                      void *stream);

/* get_valid_flag (kitti_rcnn_dataset.py:201-222) + Calibration.lidar_to_rect / rect_to_img (calibration.py:51-71) for whole
 * batches -- the front half of prcnn_input_stage as an operator, same arguments.  -> cls (b,n_max) u8: 0 = not valid,
 * 1 = valid and z < far_depth, 2 = valid beyond (rows >= counts[b]: 0); rect (b,n_max,3) f32 rectified coordinates (may be
 * NULL).  Bit-identical to the reference's numpy results: float32 np.dot is a chain of fused multiply-adds over the inner
 * index, which the kernel reproduces (tests/golden g11, recorded by running the reference's code). */
int prcnn_valid_flags(int b, int n_max, int stride, int lidar_frame, int image_filter, const int *counts, const float *raw,
                      const float *calib, const double *scope_host, float far_depth, float *rect, unsigned char *cls,
                      void *stream);

/* ---- evaluate/eval2.py: host-side matching of the AP evaluator (HOST pointers, f64 / i64) ---- */

/* compute_statistics_jit  evaluate/eval2.py:170-289 for one image.  overlaps (n_dt,n_gt) row-major,
 * gt_datas (n_gt,5) = [bbox x4, alpha], dt_datas (n_dt,6) = [bbox x4, alpha, score], ignored_* in {-1,0,1},
 * dc_bboxes (n_dc,4).  -> tp_fp_fn[3], similarity, thresholds (room for n_gt) and their count. */
int prcnn_kitti_image_stats(int n_gt, int n_dt, int n_dc, const double *overlaps, const double *gt_datas,
                            const double *dt_datas, const long long *ignored_gt, const long long *ignored_det,
                            const double *dc_bboxes, int metric, double min_overlap, double thresh, int compute_fp,
                            int compute_aos, long long *tp_fp_fn, double *similarity, double *thresholds,
                            int *n_thresholds);

/* First pass of eval_class (evaluate/eval2.py:512-527) over all images: scores of matched detections
 * (compute_fp = False, thresh = 0).  Per-image arrays are concatenated; overlaps_flat holds the (n_dt,n_gt)
 * blocks back to back.  scores_out has room for sum(gt_nums). */
int prcnn_kitti_collect_scores(int n_img, const long long *gt_nums, const long long *dt_nums,
                               const double *overlaps_flat, const double *gt_datas, const double *dt_datas,
                               const long long *ignored_gts, const long long *ignored_dets, int metric,
                               double min_overlap, double *scores_out, long long *n_scores);

/* fused_compute_statistics  evaluate/eval2.py:300-349 over all images:
 * pr (n_thresh,4) += [tp, fp, fn, similarity] at every score threshold. */
int prcnn_kitti_accumulate_pr(int n_img, const long long *gt_nums, const long long *dt_nums, const long long *dc_nums,
                              const double *overlaps_flat, const double *gt_datas, const double *dt_datas,
                              const double *dontcares, const long long *ignored_gts, const long long *ignored_dets,
                              int metric, double min_overlap, const double *thresholds, int n_thresh, int compute_aos,
                              double *pr);

/* (1 + cos(gt alpha - dt alpha)) / 2 of every (detection j, ground-truth i) pair of every image, written at
 * pair_off[image] + j * n_gt + i -- the overlap blocks' layout -- by the very cosine call prcnn_kitti_image_stats sums.  HOST
 * pointers; gt_off / dt_off / pair_off (n_img + 1) i64 prefix offsets.  The device pass (prcnn_ap_pr) only ADDS these terms: a device
 * cosine need not agree with libm's in the last bit, and the orientation similarity is compared bit for bit. */
int prcnn_kitti_pair_cos(int n_img, const long long *gt_off, const long long *dt_off, const long long *pair_off,
                         const double *gt_alpha, const double *dt_alpha, double *out);

/* ---- evaluate/eval2.py: the same statistics on the device (csrc/kitti_ap.hip; DEVICE pointers unless said otherwise) ----
 *
 * Contract: every stage gives the bits of its host definition -- kitti_eval.split_flags / clean_data, calculate_iou, the host entries
 * above, kitti_eval.thresholds_loop -- for any input without NaNs.  Nothing is read back between the stages; all launches go to
 * `stream`.
 *
 * The split table: the concatenated columns of all images (kitti_eval.SplitTable).  Offsets are (n_img + 1) i64 prefix sums; pair_off
 * counts n_dt x n_gt per image and a pair (j, i) of image m lives at pair_off[m] + j * n_gt_m + i.  Class codes are i8: 0 car,
 * 1 pedestrian, 2 cyclist, 3 van, 4 person_sitting, -1 anything else (lower-cased names).  dc_bbox holds the rows named exactly
 * "DontCare", image by image.  *_box3d (n,7) f64 = location x y z, dimensions l h w, rotation_y; *_bev (n,5) f32 = x z l w ry.
 * max_dt = the largest n_dt of an image; ws_slot (n_img) i32 = rank of the image among those with n_dt > PRCNN_AP_REG_DETS, in image
 * order (unread for the others): such an image keeps its scan flags in the workspace, any n_dt works.  Every entry below takes
 * the table as `split` (HOST words, see the index enum). */
enum { PRCNN_AP_SAMPLE_PTS = 41, PRCNN_AP_REG_DETS = 128 };
/* The table is handed over as a HOST array of PRCNN_AP_SPLIT_WORDS i64 words: the counts, then the DEVICE pointers, at these indices. */
enum { PRCNN_AP_N_IMG = 0, PRCNN_AP_MAX_DT, PRCNN_AP_N_GT, PRCNN_AP_N_DT, PRCNN_AP_N_DC, PRCNN_AP_N_PAIR,
       PRCNN_AP_GT_OFF, PRCNN_AP_DT_OFF, PRCNN_AP_DC_OFF, PRCNN_AP_PAIR_OFF,      /* (n_img + 1) i64 each */
       PRCNN_AP_WS_SLOT,                                                          /* (n_img) i32 */
       PRCNN_AP_GT_CODE, PRCNN_AP_DT_CODE,                                        /* i8 */
       PRCNN_AP_GT_OCCLUDED, PRCNN_AP_GT_TRUNCATED, PRCNN_AP_GT_BBOX, PRCNN_AP_GT_DEPTH, PRCNN_AP_GT_BOX3D,      /* f64 */
       PRCNN_AP_DT_BBOX, PRCNN_AP_DT_DEPTH, PRCNN_AP_DT_SCORE, PRCNN_AP_DT_BOX3D, PRCNN_AP_DC_BBOX,              /* f64 */
       PRCNN_AP_GT_BEV, PRCNN_AP_DT_BEV,                                          /* f32 */
       PRCNN_AP_SPLIT_WORDS };

/* clean_data (eval2.py:28-98; metric_old: eval_old.py:28-91) of the whole split for n_diff <= 8 difficulties in one launch.
 * cls / sibling: class codes (sibling -2: none).  caps HOST (n_diff,5) f64 = max occlusion, max truncation, band near, band far,
 * minimum bbox height.  -> ignored_gt (n_diff,n_gt) / ignored_dt (n_diff,n_dt) i8 in {-1,0,1}, num_valid_gt (n_diff) i32. */
int prcnn_ap_flags(const long long *split, int cls, int sibling, int metric_old, int n_diff, const double *caps,
                   char *ignored_gt, char *ignored_dt, int *num_valid_gt, void *stream);

/* Overlap blocks in f64, flat (n_pair): kind 0 image_box_overlap(dt, gt, -1); kind 2 the 3D overlap from rinc (n_pair) f32, the
 * criterion-2 output of prcnn_rotate_iou_eval_segmented over dt_bev / gt_bev (kind 1 is that launch with criterion -1, widened). */
int prcnn_ap_overlaps(const long long *split, int kind, const float *rinc, double *out, void *stream);

/* Pass 1 for every (image, group), group = difficulty * n_lev + level; min_overlaps (n_lev) f64; overlaps (n_pair) f64.
 * -> scores (n_groups,n_gt): the matched detection's score in the slot of its ground-truth box, -inf elsewhere; valid (n_groups,n_gt)
 * i8 marks.  workspace: workspace_words >= ceil(max_dt / 64) u64 words per (image with a ws_slot, group); unused (may be NULL) when
 * max_dt <= PRCNN_AP_REG_DETS. */
int prcnn_ap_scores(const long long *split, const char *ignored_gt, const char *ignored_dt, int n_diff, int n_lev,
                    const double *min_overlaps, const double *overlaps, int kind, double *scores, char *valid,
                    unsigned long long *workspace, long long workspace_words, void *stream);

/* get_thresholds (eval2.py:8-25) per group on its row of sorted_scores (n_groups,n_gt_total), descending, the first count[g] valid;
 * num_valid_gt (n_groups / n_lev) i32.  -> thresholds (n_groups,41) f64, n_thr (n_groups) i32 (what the loop takes; > 41 is stored
 * up to 41 only). */
int prcnn_ap_thresholds(int n_groups, int n_lev, long long n_gt_total, const double *sorted_scores, const int *count,
                        const int *num_valid_gt, double *thresholds, int *n_thr, void *stream);

/* Pass 2 + sums: image_stats with compute_fp for every (image, group, threshold < n_thr) and pr (n_groups,41,4) f64 =
 * [tp, fp, fn, similarity].  counts (n_groups,41,3) u64 scratch (cleared here).  Orientation: pair_cos (n_pair) from
 * prcnn_kitti_pair_cos and sim_img (n_img,n_groups,41) f64 scratch, both or neither; per-image sums add in ground-truth order, the
 * total in image order.  workspace: 2 x 64 x workspace_words u64 words per (image with a ws_slot, group). */
int prcnn_ap_pr(const long long *split, const char *ignored_gt, const char *ignored_dt, int n_diff, int n_lev,
                const double *min_overlaps, const double *overlaps, int kind, const double *thresholds, const int *n_thr,
                const double *pair_cos, unsigned long long *counts, double *sim_img, double *pr,
                unsigned long long *workspace, long long workspace_words, void *stream);

/* ---- evaluate/kitti_common.py:306-360: the label / result TEXT of one split side to columns (csrc/kitti_parse.hip; DEVICE pointers) ----
 *
 * text (n_bytes <= PRCNN_PARSE_MAX_BYTES) holds the bytes of all files, one behind the other; file_off (n_files + 1) i64.  A line is
 * what readlines() yields, stripped of spaces at both ends.  A file is REGULAR when it is empty or every line of it has the same
 * 15 or 16 tokens divided by single spaces, every byte is '\n', a space or 0x21 .. 0x7e, token 2 is [+-]?[0-9]{1,15} and tokens 1,
 * 3 .. 15 are [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]{1,9})? with at most 15 digits from the first non-zero one to the
 * last one written and |k| <= 22, k = exponent - fraction digits.  Such a token's value is the digits as an integer w times 10^k
 * (k >= 0) or over 10^-k: one correctly rounded f64 operation on exact operands, sign last -- Python's float(token), bit for bit.
 * Every other file is FLAGGED, its rows are not to be used, and the host parser reads it.  With skip_blank a line of spaces
 * alone is a row with row_tok 0 that the caller drops; without, it flags its file.
 * Columns of a row, in f64: */
enum { PRCNN_PARSE_OCCLUDED = 0, PRCNN_PARSE_TRUNCATED, PRCNN_PARSE_ALPHA, PRCNN_PARSE_BBOX, PRCNN_PARSE_LOCATION = 7,
       PRCNN_PARSE_DIMENSIONS = 10 /* l, h, w from file order h, w, l */, PRCNN_PARSE_ROTATION_Y = 13,
       PRCNN_PARSE_SCORE /* 0 in a 15-token row */, PRCNN_PARSE_COLS };
enum { PRCNN_PARSE_CHUNK = 4096, PRCNN_PARSE_MAX_BYTES = 2147483647 };
/* file_flag bits; a file is regular when its word is 0 (no row), PRCNN_PARSE_SAW15 or PRCNN_PARSE_SAW16 */
enum { PRCNN_PARSE_SAW15 = 1, PRCNN_PARSE_SAW16 = 2, PRCNN_PARSE_BAD = 4 };

/* Scan: -> row_off (n_files + 1) i64, the lines of the files as prefix sums (the caller reads them back: row_off[n_files] sizes the
 * outputs of prcnn_kitti_parse_rows).  Scratch that the second call reads again: start_flag (n_bytes) u8 and chunk_rows
 * (ceil(n_bytes / PRCNN_PARSE_CHUNK) + 1) i32. */
int prcnn_kitti_parse_scan(long long n_bytes, int n_files, const unsigned char *text, const long long *file_off,
                           unsigned char *start_flag, int *chunk_rows, long long *row_off, void *stream);

/* Parse: n_rows = row_off[n_files].  -> row_start (n_rows) i32 scratch; vals (n_rows, PRCNN_PARSE_COLS) f64; name_span (n_rows, 2) i32 =
 * offset in text and length of the name token; code (n_rows) i8 class code of the lower-cased name (the split table's codes);
 * is_dc (n_rows) u8: the name is exactly "DontCare"; row_tok (n_rows) u8: 15, 16, or 0 for a row that is blank or not regular
 * (its other columns are zero); file_flag (n_files) i32 (cleared here). */
int prcnn_kitti_parse_rows(long long n_bytes, int n_files, long long n_rows, int skip_blank, const unsigned char *text,
                           const long long *file_off, const unsigned char *start_flag, const int *chunk_rows,
                           const long long *row_off, int *row_start, double *vals, int *name_span, char *code,
                           unsigned char *is_dc, unsigned char *row_tok, int *file_flag, void *stream);

/* Statistical normalization (stat_norm/norm.py:186-330 rescale_ptc) over a batch of ragged scenes (csrc/stat_norm.hip).
 * Device pointers; offsets are prefix sums over the scenes (n_scenes + 1 entries).  Points: velo (sum n, 4) f32 raw .bin rows,
 * pt_off; 64-point tiles: tile_off; rescaled boxes: box_off, boxd (n_box, PRCNN_SN_BOXD) f64 records, boxi (n_box, PRCNN_SN_BOXI) i32 state (zeroed),
 * mm (n_box, 6) f64 min xyz / max xyz (+inf / -inf; avoid_conflict only); bt_cnt (sum nbox * ntile) i32 at bt_off per scene;
 * rem_cnt (sum ntile) i32; scene_i (n_scenes, 4) i32 = [remainder, patch points, output points, -]; calib (n_scenes, 42) f64 =
 * V2C, R0, inv(R0), C2V; out_off / out (sum n_out, 4) f32 for the write pass. */
/* a boxd record, in doubles: what the host fills -- translation, rotation (3 x 3 row-major) and the box-frame bounds before the count pass,
 * with avoid_conflict the 11 x 3 candidate scales (l, h, w axis order = box-frame x, y, z); before the write pass the chosen scale, the two
 * align_front shifts (x, z each) and their flags */
enum {
    PRCNN_SN_T = 0, PRCNN_SN_R = 3, PRCNN_SN_XLO = 12, PRCNN_SN_XHI, PRCNN_SN_YLO, PRCNN_SN_ZLO, PRCNN_SN_ZHI, PRCNN_SN_SCALE = 17,
    PRCNN_SN_FSCALE = 50, PRCNN_SN_SHIFT = 53, PRCNN_SN_FLAG1 = 57, PRCNN_SN_FLAG2 = 58, PRCNN_SN_BOXD = 64
};
/* a boxi record, in ints: what the host reads after the choose pass -- the inside count and the ratio index -- and the record's width */
enum { PRCNN_SN_CNT = 0, PRCNN_SN_RIDX = 13, PRCNN_SN_BOXI = 16 };
typedef struct prcnn_sn_batch {
    int n_scenes, max_tiles, max_boxes, avoid;
    const int *pt_off, *tile_off, *box_off;
    const long long *bt_off;
    const float *velo;
    const double *calib, *boxd;
    int *boxi;
    double *mm;
    int *bt_cnt, *rem_cnt, *scene_i;
    const long long *out_off;
    float *out;
} prcnn_sn_batch;
/* pass 1: inside counts per (box, tile) -> ordered exclusive offsets, inside totals, env_mask0 counts, min / max, remainder */
int prcnn_stat_norm_count(const prcnn_sn_batch *batch, void *stream);
/* pass 2: (avoid_conflict) 11 env counts per box; then per box the ratio index (-1 = ratio 0, 0..10 = np.arange(1, -0.1, -0.1))
 * and patch base, per scene the output size */
int prcnn_stat_norm_choose(const prcnn_sn_batch *batch, void *stream);
/* pass 3: the output clouds (x, y, z, 1) f32, boxd's write-pass fields (chosen scale, align_front shifts) filled by the host */
int prcnn_stat_norm_write(const prcnn_sn_batch *batch, void *stream);
/* postprocessing's occlusion map: rects (n_obj, 4) i32 = half-open [y0, y1) x [x0, x1) per object in painting order, obj_off per
 * scene; counts (n_obj) i32 (zeroed) += pixels whose last painter is the object.  At most 2048 objects per scene. */
int prcnn_stat_norm_occlusion(int n_scenes, int h, int w, int max_objects, const int *obj_off, const int *rects, int *counts,
                              void *stream);

/* RPN labels (kitti_rcnn_dataset.py:385-414 generate_rpn_training_labels) for a batch of ragged scenes (csrc/rpn_labels.hip).
 * pts (b, n, 3) f32 rect frame; gt (b, g, 7) f32 [x, y_bottom, z, h, w, l, ry] with counts (b) i32 valid rows per scene; trig (b, g, 2)
 * f32 = numpy's f32 (cos ry, sin ry); scores (b, n) raw RPN scores or NULL; cls (b, n) i32 -1 / 0 / 1; reg (b, n, 7) f32 or NULL;
 * stats (b, 3) i32 (zeroed by the caller) += (correct, fg, pred) or NULL; work: prcnn_rpn_labels_workspace bytes (may be NULL if g = 0). */
int prcnn_rpn_labels_workspace(int b, int g, long long *bytes);
int prcnn_rpn_labels(int b, int n, int g, const float *pts, const float *gt, const int *counts, const float *trig, const float *scores,
                     float thresh, int *cls, float *reg, int *stats, double *work, void *stream);

/* GT-database point extraction (tools/generate_gt_database.py:59-87) for a batch of ragged scenes (csrc/gt_database.hip).
 * pt_off / tile_off / box_off (n_scenes + 1) i32: points, 64-point tiles and boxes per scene, back to back; bt_off (n_scenes + 1) i64
 * into bt_cnt (sum n_box * n_tile) i32; velo (sum n, 4) f32 raw points; calib (n_scenes, 12) f32 = np.dot(V2C.T, R0.T), (4, 3)
 * row-major; boxes (sum g, 7) f32 [x, y_bottom, z, h, w, l, ry]; trig (sum g, 2) f32 from prcnn_gt_box_trig; counts (sum g) i32
 * (zeroed by the caller) = points inside every box; out_off (sum g + 1) i64 = exclusive sums of counts; out (sum counts, 4) f32 =
 * rect x, y, z | intensity, every object's rows in point-index order.  max_tiles / max_boxes: the largest scene's. */
typedef struct prcnn_gt_batch {
    int n_scenes, max_tiles, max_boxes, reserved;
    const int *pt_off, *tile_off, *box_off;
    const long long *bt_off;
    const float *velo, *calib, *boxes, *trig;
    int *bt_cnt, *counts;
    const long long *out_off;
    float *out;
} prcnn_gt_batch;
/* boxes per LDS chunk of the kernels (the tests place their box counts around it) */
int prcnn_gt_box_chunk(void);
/* HOST pointers: trig (n, 2) f32 = (cos ry, sin ry) as prcnn_host_pts_in_boxes3d evaluates them */
int prcnn_gt_box_trig(int n, const float *boxes3d, float *trig);
/* passes 1 + 2: inside counts per (box, tile) -> ordered exclusive offsets in bt_cnt, totals in counts */
int prcnn_gt_extract_count(const prcnn_gt_batch *batch, void *stream);
/* pass 3: the objects' rows (out_off / out set by the caller from the totals) */
int prcnn_gt_extract_write(const prcnn_gt_batch *batch, void *stream);

/* Augmented-scene generation (tools/generate_aug_scene.py:150-249) for a batch of ragged scenes and of jobs = (epoch, scene) pairs
 * over them (csrc/aug_scene.hip).  Device pointers.  Scenes: pt_off / tile_off / box_off (n_scenes + 1) i32 as in prcnn_gt_batch; velo
 * (sum n, 4) f32 raw points; calib (n_scenes, PRCNN_CALIB_ROW) f32 = V2C | R0 | P2 | image height, width (prcnn_valid_flags' layout); scope 6 f64
 * x0, x1, y0, y1, z0, z1 (PC_AREA_SCOPE); boxes (sum g, 7) f32 = the scenes' non-DontCare label boxes; rect (sum n, 4) f32 and valid
 * (sum n) u8: the filter's results (rect x, y, z | intensity; valid flag).  Jobs: job_scene (n_jobs) i32; jt_off (n_jobs + 1) i64 into
 * tile_cnt (sum of the jobs' scenes' tiles) i32; cand_n (n_jobs) i32 <= 16 candidates in try order with cand_db (n_jobs, 16) i32 =
 * database entry, cand_box (n_jobs, 16, 7) f32 = its box on the road plane, cand_trig (n_jobs, 16, 2) f32 from prcnn_gt_box_trig,
 * cand_move (n_jobs, 16) f64 = move_height; sizes (n_jobs, 18) i32 = [kept points, accepted, the accepted slots in acceptance order
 * (-1 behind them)].  Database: db_pts (sum m, 4) f32 rect x, y, z | intensity, db_off (n_db + 1) i64.  Output: out_off (n_jobs + 1) i64
 * rows per job, obj_off (n_jobs, 17) i64 = first row of every accepted object (and the end of the last), out (rows, 4) f32 = the kept
 * points in point order, then the accepted objects' points.  max_tiles: the largest scene's. */
typedef struct prcnn_aug_batch {
    int n_scenes, n_jobs, max_tiles, n_db;
    const int *pt_off, *tile_off, *box_off;
    const float *velo, *calib;
    const double *scope;
    const float *boxes;
    float *rect;
    unsigned char *valid;
    const int *job_scene;
    const long long *jt_off;
    const int *cand_n, *cand_db;
    const float *cand_box, *cand_trig;
    const double *cand_move;
    int *sizes, *tile_cnt;
    const float *db_pts;
    const long long *db_off, *out_off, *obj_off;
    float *out;
} prcnn_aug_batch;
/* candidates per job (16) */
int prcnn_aug_max_candidates(void);
/* filter, placement, kept counts: fills rect, valid, tile_cnt (ordered exclusive offsets) and sizes */
int prcnn_aug_place(const prcnn_aug_batch *batch, void *stream);
/* the rows (out_off / obj_off / out set by the caller from sizes) */
int prcnn_aug_write(const prcnn_aug_batch *batch, void *stream);

/* RPN training input stage (lib/datasets/kitti_rcnn_dataset.py:249-382 get_rpn_sample in TRAIN mode, GT-aug :428-531 and
 * data_augmentation :533-591 included) for a batch of ragged scenes (csrc/train_input.hip).  Device pointers.  Scenes: pt_off /
 * tile_off / box_off (n_scenes + 1) i32 as in prcnn_aug_batch; velo (sum n, 4) f32 raw points, or rect x, y, z | intensity where
 * is_rect (n_scenes) u8 is set; calib (n_scenes, PRCNN_CALIB_ROW) f32 and scope 6 f64 as in prcnn_aug_batch, the scope applied when reduce_by_range;
 * box_rec (sum g, PRCNN_TR_REC) f64 = the overlap records of the scenes' non-DontCare boxes (w, l + 0.5): the four BEV corners x, z of the f32
 * corner array, min_h, max_h, the f32 volume term; cand_n (n_scenes) i32, cand_rec (n_scenes, 16, PRCNN_TR_REC) f64 the candidates' records,
 * cand_box (n_scenes, 16, 7) f32 placed boxes, cand_trig (n_scenes, 16, 2) f32, cand_move (n_scenes, 16) f64 = move_height.
 * Work: rect (sum n, 4) f32, valid and flag (sum n) u8 (flag: bit 0 kept, bit 1 near), tile_cnt (2 * tiles) i32 interleaved kept /
 * near ordered exclusive offsets, lists (3, sum n) i32 = the kept / near / far points' indices in point order.  sizes (n_scenes, 19)
 * i32 = [kept points, near kept points, accepted, the accepted slots in acceptance order (-1 behind them)]: the block the host reads.
 * Emit: db_pts (n_db_rows, 4) f32 resident rect x, y, z | intensity; codes (n_scenes, npoints) i64 = kind << 56 | slot << 48 | value
 * with kind 0 / 1 / 2 (PRCNN_TR_KEPT / NEAR / FAR) a rank in the kept / near / far list and kind 3 (PRCNN_TR_DB) a database row whose object sits in candidate slot `slot`; aug
 * (n_scenes, 6) f64 = rotmat.T as m00, m10, m01, m11, the f32 scale, flags (1 rotation, 2 scaling, 4 flip); pts_rect (n_scenes,
 * npoints, 3), pts_input (n_scenes, npoints, input_channels = 3 | 4), pts_features (n_scenes, npoints, 1) f32.  max_tiles: the largest tile count among the scenes
 * [scene_begin, scene_end) of a place call (it sizes the grid). */
enum { PRCNN_TR_REC = 11 };   /* doubles per overlap record */
/* an emit code: kind << PRCNN_TR_KIND_SHIFT | slot << PRCNN_TR_SLOT_SHIFT | value (the bits below the slot) */
enum { PRCNN_TR_KEPT = 0, PRCNN_TR_NEAR, PRCNN_TR_FAR, PRCNN_TR_DB, PRCNN_TR_SLOT_SHIFT = 48, PRCNN_TR_KIND_SHIFT = 56 };
typedef struct prcnn_train_batch {
    int n_scenes, max_tiles, npoints, input_channels, reduce_by_range, scene_begin, scene_end, reserved;
    long long n_db_rows;
    const int *pt_off, *tile_off, *box_off;
    const float *velo, *calib;
    const double *scope;
    const unsigned char *is_rect;
    const double *box_rec;
    const int *cand_n;
    const double *cand_rec;
    const float *cand_box, *cand_trig;
    const double *cand_move;
    float *rect;
    unsigned char *valid, *flag;
    int *tile_cnt, *lists, *sizes;
    const float *db_pts;
    const long long *codes;
    const double *aug;
    float *pts_rect, *pts_input, *pts_features;
} prcnn_train_batch;
/* filter, placement under the online overlap rule, flags, ordered scans, index lists of the scenes [scene_begin, scene_end): fills
 * their part of rect .. lists and sizes.  (The sampler's draws of scene i come before the GT-aug draws of scene i + 1 in the loader's
 * stream and their number depends on scene i's counts, so a caller that owns that stream places scene by scene.) */
int prcnn_train_place(const prcnn_train_batch *batch, void *stream);
/* the B x npoints output rows (codes / aug / outputs set by the caller after it has read sizes) */
int prcnn_train_emit(const prcnn_train_batch *batch, void *stream);

/* Random object scaling of a training batch (csrc/object_scale.hip, object_scale.py; the project's own definition).  Device pointers.
 * pts (b, n, 3) f32 rect points, scaled in place; extra (b, n, extra_channels = 3 | 4) f32 or NULL: its columns 0..2 receive the same
 * written values (a fourth column is never touched); gt (b, g, 7) f32 [x, y_bottom, z, h, w, l, ry] with counts (b) i32 valid rows per
 * scene; trig (b, g, 2) f32 = numpy's f32 (cos ry, sin ry); factors (b, g) f64; hits (b, g) u32 (zeroed by the caller) += the points
 * that box k owns.  The owner of a point is the lowest k < counts[s] with |a| <= l / 2, |b| <= w / 2, 0 <= v <= h for dx = px - x,
 * dz = pz - z, v = y - py, a = dx cos - dz sin, b = dx sin + dz cos (f64, faces inclusive); with r = factors[s, owner] != 1 the point
 * becomes (x + (a r cos + b r sin), y - v r, z + (b r cos - a r sin)) rounded to f32, otherwise its bits are kept.  The boxes are not
 * written.  b = 0 or n = 0 returns before any launch; g = 0 launches nothing. */
int prcnn_object_scale(int b, int n, int g, float *pts, float *extra, int extra_channels, const float *gt, const int *counts,
                       const float *trig, const double *factors, unsigned int *hits, void *stream);

/* RCNN training targets (lib/rpn/proposal_target_layer.py; csrc/rcnn_targets.hip, rcnn_targets.py).  Device pointers.
 * (a) rois (b, m, 7), gt (b, g, 7) with trailing zero-sum rows -> per RoI the row maximum of the 3-D IoU (max_ov), the first index
 * that attains it (assign), its list cls (b, m) u8 (0 fg: >= fg_thresh, 1 hard bg: [bg_lo, bg_thresh), 2 easy bg: < bg_lo, 3 none);
 * lists (b, 3, m) i32 the three ascending index lists; sizes (b, 4) i32 = their lengths and the ground-truth rows that remain: the
 * block the host reads.  Work: tile_cnt (b, 3, ceil(m / 64)) i32. */
int prcnn_rcnn_assign(int b, int m, int g, const float *rois, const float *gt, float fg_thresh, float bg_thresh, float bg_lo,
                      float *max_ov, int *assign, unsigned char *cls, int *tile_cnt, int *lists, int *sizes, void *stream);
/* sampled RoIs per scene (128) and tries per RoI (64) that prcnn_rcnn_aug_rois holds */
int prcnn_rcnn_max_rois(void);
int prcnn_rcnn_max_tries(void);
/* (b) the noise tries of ONE scene's n_rois sampled RoIs, the first n_fg of them foreground (fg_times tries at most, the others
 * bg_times = 0 | 1).  rois (m, 7), gt (g, 7), max_ov / assign (m), lists (3, m): the scene's part of (a)'s arrays; pick (n_rois, 2) i32
 * = (list, position in it) of every sampled RoI.  The pools, indexed by the position in the scene's numpy try stream: keep (n_pool)
 * u8 = the draw was < 0.2 (the RoI itself is tried), noise (n_pool, 8) f32 = the noise level and the seven uniforms the try at that
 * position reads from the torch stream; method 0 'single', 1 'multiple'.  Work: table (n_fg, n_pool) f32.  Out: out_rois the tried
 * boxes that stay, out_pool_rois the same enlarged by pool_extra_width, out_gt (n_rois, 7) their ground truth, out_iou the gt_iou rule,
 * out_src the source RoI, out_cnt / out_keep the try count and the last try's keep flag, out_tried (n_rois, max(fg_times, bg_times, 1))
 * every tried IoU (NaN behind them), used[0] = the numpy draws consumed. */
typedef struct prcnn_rcnn_aug {
    int m, g, n_rois, n_fg, fg_times, bg_times, method, n_pool;
    float pos_thresh, pool_extra_width;
    const float *rois, *gt, *max_ov;
    const int *assign, *lists, *pick;
    const unsigned char *keep;
    const float *noise;
    float *table;
    float *out_rois, *out_pool_rois, *out_gt, *out_iou;
    int *out_src, *out_cnt, *out_keep;
    float *out_tried;
    int *used;
} prcnn_rcnn_aug;
int prcnn_rcnn_aug_rois(const prcnn_rcnn_aug *args, void *stream);
/* (c) one pass over the pooled rows: pooled (rows, s, cin) f32 and empty (rows) i32 as prcnn_roipool3d leaves them, rows = scenes x
 * sampled RoIs; aug_rand (3, rows) f32 the rotation / scale / flip uniforms (read when aug_data), rot_scale = pi / AUG_ROT_RANGE ->
 * rois_out, gt_out (rows, 7) (augmented RoI; target box in the RoI's canonical frame), sampled_pts (rows, s, 3), pts_feature
 * (rows, s, cin - 3), cls_label and reg_valid (rows) i64. */
typedef struct prcnn_rcnn_target_args {
    int rows, s, cin, aug_data;
    float rot_scale, reg_fg, cls_fg, cls_bg;
    const float *pooled;
    const int *empty;
    const float *aug_rand, *rois_in, *gt_in, *gt_iou;
    float *rois_out, *gt_out, *sampled_pts, *pts_feature;
    long long *cls_label, *reg_valid;
} prcnn_rcnn_target_args;
int prcnn_rcnn_targets(const prcnn_rcnn_target_args *args, void *stream);

/* Training losses of both stages with their gradients (lib/net/train_functions.py get_rpn_loss / get_rcnn_loss, lib/utils/loss_utils.py;
 * csrc/losses.hip, losses.py).  Device pointers.  n classification entries = n regression rows of c channels.  One stage's loss is the
 * three calls below in this order on one stream, with no host read between them; every sum goes through per-block partials in `work`
 * that are combined in a fixed order (no floating-point atomics: the same input gives the same bits).
 *   label (n) i64: -1 ignored, 0 background, > 0 foreground; reg_mask (n) i64 or NULL: the regression rows are reg_mask > 0 (NULL:
 *   label > 0); cls (n) logits; reg (n, c); reg_label (n, 7) = dx dy dz h w l ry; anchors NULL (the anchor is anchor[3]) or (n, 7)
 *   boxes whose [3:6] is the row's anchor.  cls_kind 0 DiceLoss, 1 SigmoidFocalLoss (alpha, gamma), 2 BinaryCrossEntropy (fg_weight).
 *   Out: grad_cls (n), grad_reg (n, c) = d loss / d cls, d loss / d reg (rows outside the mask: zeros, written without reading reg),
 *   parts (PRCNN_LOSS_PARTS) f32, the layout below.  work: prcnn_loss_workspace() doubles.
 * Decisions (bin labels, the heading's fold, BCE's sigmoid and clamps) are taken in f32 exactly as the reference's operators take
 * them; the arithmetic on top of them and every sum run in f64 and are rounded to f32 once. */
enum { PRCNN_LOSS_DICE = 0, PRCNN_LOSS_FOCAL = 1, PRCNN_LOSS_BCE = 2 };
enum {
    PRCNN_LP_LOSS = 0, PRCNN_LP_CLS, PRCNN_LP_REG, PRCNN_LP_LOC, PRCNN_LP_ANGLE, PRCNN_LP_SIZE /* x 3 */, PRCNN_LP_CLS_POS, PRCNN_LP_CLS_NEG,
    PRCNN_LP_X_BIN, PRCNN_LP_Z_BIN, PRCNN_LP_X_RES, PRCNN_LP_Z_RES, PRCNN_LP_Y_BIN, PRCNN_LP_Y_RES, PRCNN_LP_Y_OFFSET, PRCNN_LP_RY_BIN,
    PRCNN_LP_RY_RES, PRCNN_LP_SIZE_RAW /* before the x 3 */, PRCNN_LP_N_POS, PRCNN_LP_N_NEG, PRCNN_LP_N_VALID, PRCNN_LP_N_REG_FG,
    PRCNN_LP_DICE_MIN, PRCNN_LP_DICE_MAX, PRCNN_LOSS_PARTS
};
typedef struct prcnn_loss_args {
    int n, c, cls_kind;
    int xz_fine, y_by_bin, ry_fine;
    int nbin_loc, nbin_y, nbin_head;
    float loc_scope, loc_bin, y_scope, y_bin;
    float alpha, gamma, fg_weight, w_cls, w_reg;
    float anchor[3];
    const float *cls;
    const long long *label, *reg_mask;
    const float *reg, *reg_label, *anchors;
    float *grad_cls, *grad_reg, *parts;
    double *work;
} prcnn_loss_args;
int prcnn_loss_workspace(void);
/* counts of pos / neg / valid / regression rows; for Dice also sum min(p, t) m and sum max(p, t) m */
int prcnn_loss_stats(const prcnn_loss_args *args, void *stream);
/* the classification loss's terms and grad_cls (normalisers read from work) */
int prcnn_cls_loss(const prcnn_loss_args *args, void *stream);
/* the bin-based regression loss's terms and grad_reg, then the one-block finish that writes parts */
int prcnn_reg_loss(const prcnn_loss_args *args, void *stream);

/* The weight step of training over every parameter tensor of a model: gradient-norm clip (torch.nn.utils.clip_grad_norm_), decoupled weight
 * decay (tools/train_utils/fastai_optim.py OptimWrapper.step) and torch.optim.Adam, in the three calls below in this order on one stream,
 * with no host read between them (csrc/optim.hip, optim.py).  The tensors are described by a table of plain DEVICE arrays:
 *   per tensor (n_tensors): param / grad / exp_avg / exp_avg_sq addresses of contiguous f32 data (0: absent), numel, flags (bit 0 "decay":
 *   param *= 1 - wd lr; bit 1 "adam": the tensor has a grad and state), step (the tensor's own Adam step count);
 *   per chunk (n_chunks): chunk_tensor and chunk_start -- a chunk is at most PRCNN_OPTIM_CHUNK consecutive elements of one tensor, every
 *   element of every tensor lies in exactly one chunk.
 * work: prcnn_optim_workspace(n_chunks) doubles; after prcnn_optim_finish work[0] is the total gradient norm over every tensor with a
 * grad address and work[1] = min(1, max_norm / (work[0] + 1e-6)).  The arithmetic runs in f64 from the f32 state and every stored value
 * is rounded to f32 once; the sums have a fixed shape (no atomics: the same input gives the same bits).  Grads are read, never written. */
enum { PRCNN_OPTIM_CHUNK = 2048 };
int prcnn_optim_workspace(int n_chunks);
/* work[2 + chunk] = sum of squares of the chunk's grads (0 where the tensor has none) */
int prcnn_optim_sumsq(const unsigned long long *grad_addr, const long long *numel, const int *chunk_tensor, const long long *chunk_start,
                      int n_tensors, int n_chunks, double *work, void *stream);
/* one workgroup: work[0], work[1]; step += 1 of every tensor flagged "adam" */
int prcnn_optim_finish(const unsigned char *flags, int *steps, int n_tensors, int n_chunks, double max_norm, double *work, void *stream);
/* g = grad work[1]; "decay": p *= 1 - wd lr; "adam": m += (g - m)(1 - beta1), v = beta2 v + (1 - beta2) g g,
 * p -= lr / (1 - beta1^step) m / (sqrt(v) / sqrt(1 - beta2^step) + eps) */
int prcnn_optim_update(const unsigned long long *param_addr, const unsigned long long *grad_addr, const unsigned long long *exp_avg_addr,
                       const unsigned long long *exp_avg_sq_addr, const long long *numel, const unsigned char *flags, const int *steps,
                       const int *chunk_tensor, const long long *chunk_start, int n_tensors, int n_chunks, double lr, double beta1,
                       double beta2, double eps, double wd, const double *work, void *stream);

/* Data-parallel training's two kernels over the same chunk table with one more per-tensor column (csrc/grad_bucket.hip, dist_train.py):
 * slot_start (n_tensors) i64, the tensor's first element in a flat layout whose slots are in table order and start at multiples of
 * PRCNN_BUCKET_ALIGN elements (dist_train.bucket_layout).  Device pointers; a tensor whose address is 0 has no slot and is skipped.
 * prcnn_grad_pack: bucket[slot_start[t] + j] = src[t][j] for every tensor, in ONE launch; src addresses of contiguous f32 data that need
 *   not be 16-byte aligned, bucket 16-byte aligned with bucket_numel elements; a chunk that would end past bucket_numel writes nothing;
 *   the padding between slots is never written.
 * prcnn_param_digest: work[0] = sum over every element of bits(p[j]) * (2 (slot_start[t] + j) + 1) mod 2^64, bits the element's 32 bits as
 *   an unsigned integer; work holds 1 + n_chunks words (work[1 + chunk] are the per-chunk partials).  Integers only. */
enum { PRCNN_BUCKET_ALIGN = 64 };
int prcnn_grad_pack(const unsigned long long *src_addr, const long long *numel, const long long *slot_start, const int *chunk_tensor,
                    const long long *chunk_start, int n_tensors, int n_chunks, float *bucket, long long bucket_numel, void *stream);
int prcnn_param_digest(const unsigned long long *param_addr, const long long *numel, const long long *slot_start, const int *chunk_tensor,
                       const long long *chunk_start, int n_tensors, int n_chunks, unsigned long long *work, void *stream);

/* Road-plane estimation for a batch of ragged LiDAR sweeps (csrc/road_planes.hip, road_planes.py): candidates in
 * the x / z range compacted in point order, RANSAC over host-drawn triples, two least-squares refits, the final inlier count and rms,
 * all in ONE call with no host read inside.  Device pointers.  pt_off / tile_off (n_scenes + 1) i32 and velo (sum n, 4) f32 as in
 * prcnn_gt_batch, calib (n_scenes, 12) f32 = np.dot(V2C.T, R0.T); draws (n_scenes, iters, 3) f64 in [0, 1); the range x0 <= x <= x1,
 * z0 <= z <= z1 in the rect frame; cos_tilt = cos(max tilt).  Work: tile_cnt (sum tiles) i32; cand_n (n_scenes) i32 = M; cand
 * (sum n, 4) f32 = rect x, y, z, 0 of a scene's candidates from row pt_off[scene]; hyp (n_scenes, iters, PRCNN_RP_HYP) f64 = unit
 * normal, d, the first point, accepted (1 / 0); part (n_scenes, G, iters) i32 with G = max(1, ceil(max_tiles / PRCNN_RP_GROUP_TILES));
 * scores (n_scenes, iters) i32 (0 where rejected); p0 (n_scenes, 4) f64; mom (n_scenes, PRCNN_RP_MOMENT_GROUPS, PRCNN_RP_MOM) f64.
 * out (n_scenes, PRCNN_RP_OUT) f64 = a, b, c, d, rms, M, best hypothesis (-1: fallback), its score, inliers of the final plane,
 * fallback (0 none, 1 fewer than 3 candidates, 2 no hypothesis accepted, 3 best score below min_inliers): the block the host reads. */
enum { PRCNN_RP_GROUP_TILES = 16, PRCNN_RP_HYP = 8, PRCNN_RP_MOMENT_GROUPS = 32, PRCNN_RP_MOM = 10, PRCNN_RP_OUT = 10 };
int prcnn_road_planes(int n_scenes, int max_tiles, int iters, const int *pt_off, const int *tile_off, const float *velo,
                      const float *calib, const double *draws, double x0, double x1, double z0, double z1, double thresh,
                      double cos_tilt, int min_inliers, double default_height, int *tile_cnt, int *cand_n, float *cand,
                      double *hyp, int *part, int *scores, double *p0, double *mom, double *out, void *stream);

/* Bird's-eye-view scene images (csrc/bev_render.hip, bev.py).  Device pointers.
 * prcnn_bev_bin (plain pointers and scalars): a ragged batch of clouds, packed as in prcnn_sn_batch: pt_off / tile_off / box_off
 *   (n_clouds + 1 entries i32), velo (sum n, 4) f32 raw .bin rows.  calib (n_clouds, PRCNN_BEV_CALIB) f64 = V2C (3, 4), R0 (3, 3) row-major; boxd (n_box, PRCNN_BEV_BOXD)
 *   f64 = the first PRCNN_BEV_BOXD doubles of a stat_norm box record (PRCNN_SN_T, PRCNN_SN_R, PRCNN_SN_XLO ..): centre, rotation made on
 *   the host, the five bounds.  A point is rect = R0 (V2C [p 1]) in f64, one rounding per operation, sums left to right; it is an object
 *   point when strictly inside any box of its cloud (f = (rect - t) R).  image (n_clouds) i32: the image a cloud is drawn into;
 *   layer_out / layer_in (sum n) u8: the layer of a point outside / inside the boxes (PRCNN_BEV_LAYERS or more: not drawn, not counted).
 *   In f32 u = (x - x0) * inv, v = (z - z0) * inv; kept iff 0 <= u < width and 0 <= v < height; counts (n_images, PRCNN_BEV_LAYERS,
 *   height, width) u32 [layer][height - 1 - floor(v)][floor(u)] += 1 and stats (n_images, PRCNN_BEV_LAYERS, 2) i32 = binned, dropped;
 *   both are zeroed inside the call.  cls (sum n) u8 = 1 for an object point, else 0; may be null.  u32 atomic adds only: the same
 *   input gives the same bits.  A cloud whose image is outside [0, n_images) is not drawn. */
enum { PRCNN_BEV_LAYERS = 3, PRCNN_BEV_CALIB = 21, PRCNN_BEV_BOXD = 17, PRCNN_BEV_BOX_CHUNK = 64, PRCNN_BEV_MAX_SIDE = 2048 };
int prcnn_bev_bin(int n_clouds, int max_tiles, int n_images, int height, int width, float x0, float z0, float inv, const int *pt_off,
                  const int *tile_off, const int *box_off, const int *image, const float *velo, const double *calib, const double *boxd,
                  const unsigned char *layer_out, const unsigned char *layer_in, unsigned int *counts, unsigned char *cls, int *stats,
                  void *stream);
/* prcnn_bev_compose: rgb (n_images, height, width, 3) u8, one result per pixel, no atomics.  segs (n_seg, PRCNN_BEV_SEG) i32 =
 *   ax, ay, bx, by, palette row, in units of 1/8 pixel (column, row measured downward; the centre of pixel (r, c) is (8 c + 4, 8 r + 4)),
 *   seg_off (n_images + 1) i32; palette (n_palette, 3) u8: row 0 the background, row 1 + 4 layer + step a layer's brightness step
 *   min(floor(log2 count), 3), the rows behind them the outline colours.  A pixel takes the LAST segment of its image within 4 line_px
 *   units of its centre (a row outside the palette is no segment), else the highest non-empty layer, else the background.
 *   int64 bounds: every endpoint coordinate must lie in [PRCNN_BEV_COORD_LO, PRCNN_BEV_COORD_HI] (the caller drops other boxes) and a
 *   pixel centre lies in [4, 16380], so a component of b - a is at most 2^15 in magnitude and one of p - a below 2^15; the dot product,
 *   |b - a|^2 and the cross product are at most 2^31, cross^2 at most 2^62 and R^2 |b - a|^2 at most 2^41 (R <= 32): no product
 *   leaves int64. */
enum { PRCNN_BEV_SEG = 5, PRCNN_BEV_SEG_CHUNK = 256, PRCNN_BEV_COORD_LO = -8192, PRCNN_BEV_COORD_HI = 24576, PRCNN_BEV_PALETTE_MAX = 64,
       PRCNN_BEV_MAX_LINE = 8 };
int prcnn_bev_compose(int n_images, int height, int width, int line_px, int n_palette, const unsigned int *counts, const int *seg_off,
                      const int *segs, const unsigned char *palette, unsigned char *rgb, void *stream);

/* LiDAR beam resampling (csrc/beam_resample.hip, beam_resample.py).  Device pointers, plain pointers and scalars
 * only.  A ragged batch packed as in prcnn_sn_batch: pt_off / tile_off (n_scenes + 1) i32, velo (sum n, 4) f32 raw .bin rows.  The three
 * entries run in this order on one stream; none reads on the host.  Every result equals beam_resample.py's device="cpu" path bit for bit.
 * prcnn_beam_hist: edges (bins + 1) f64, strictly increasing (the host's table).  Per point (x, y, z) = f32 coordinates as f64 minus the
 *   origin, rho2 = x x + y y (products and sum rounded separately), t = z / sqrt(rho2); point_bin (sum n) i32 = the largest i with
 *   edges[i] <= t, or -1 (unassigned) for a non-finite coordinate, rho2 == 0, t < edges[0] or t >= edges[bins].  hist (n_scenes, bins)
 *   u32, zeroed inside the call, filled with u32 atomic adds.  bins <= PRCNN_BEAM_MAX_BINS: table and histogram stay in LDS.
 * prcnn_beam_lloyd: 1-D Lloyd on each scene's histogram with `beams` clusters (<= PRCNN_BEAM_MAX_K).  Centres start at
 *   lo + k (hi - lo) / (beams - 1) (lo for one beam), lo / hi the lowest / highest occupied bin; an occupied bin goes to the nearest
 *   centre, the lower one of equals; a centre becomes (sum count * bin) / (sum count) (integer sums, one f64 division), an empty cluster
 *   keeps its own; it stops when no bin changes cluster or after PRCNN_BEAM_MAX_ITERS updates.  table (n_scenes, bins) i32 = a bin's
 *   cluster (-1: no point in it), centres (n_scenes, beams) f64, counts (n_scenes, beams) u32 points per cluster, iters (n_scenes) i32
 *   updates made, flags (n_scenes) i32 = PRCNN_BEAM_HIT_CAP | PRCNN_BEAM_UNSORTED (the centres left their order: never, by construction).
 *   A scene with no assigned point: table -1, centres and counts 0, iters 0.
 * prcnn_beam_select: beam_id (sum n) i32 = table[point_bin] (-1 unassigned); a row is kept when keep_beam[beam_id] (beams bytes) is
 *   non-zero, an unassigned one when keep_unassigned is.  Count / scan / ordered write over the 64-point tiles: tile_cnt (sum tiles) i32
 *   work, kept_n (n_scenes) i32, rows (sum n, 4) f32 = a scene's kept rows in their order from row pt_off[scene], each copied as four
 *   32-bit words. */
enum { PRCNN_BEAM_MAX_BINS = 4096, PRCNN_BEAM_MAX_K = 128, PRCNN_BEAM_MAX_ITERS = 64, PRCNN_BEAM_HIST_TILES = 64, PRCNN_BEAM_HIT_CAP = 1,
       PRCNN_BEAM_UNSORTED = 2 };
int prcnn_beam_hist(int n_scenes, int max_tiles, int bins, const int *pt_off, const float *velo, const double *edges, double ox, double oy,
                    double oz, int *point_bin, unsigned int *hist, void *stream);
int prcnn_beam_lloyd(int n_scenes, int bins, int beams, const unsigned int *hist, int *table, double *centres, unsigned int *counts,
                     int *iters, int *flags, void *stream);
int prcnn_beam_select(int n_scenes, int max_tiles, int bins, int beams, const int *pt_off, const int *tile_off, const float *velo,
                      const int *point_bin, const int *table, const unsigned char *keep_beam, int keep_unassigned, int *beam_id,
                      int *tile_cnt, int *kept_n, float *rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
