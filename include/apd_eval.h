/*
 * apd_eval.h — C-ABI of the device-side point-cloud evaluation (libapd_hip.so).
 *
 * The reference hands accuracy / completeness / F1 to an external evaluator binary
 * (tools/eval_eth_train.py). This ABI computes the part of that which is heavy: for every point of
 * one cloud the distance to the nearest point of another, truncated at max_dist, plus a voxel
 * down-sampling of a cloud. It is the plain nearest-neighbour definition (DTU-style); the ETH3D
 * tool's free-space and visibility handling is not modelled. A z-buffer renderer of a cloud into
 * cameras and a per-point visibility count against depth maps serve a plain visibility filter.
 * A scanner free-space test and voxel-averaged scores, modelled on the ETH3D protocol with a contract
 * of their own, are declared after them (parity with the ETH3D tool is not pinned). A crop volume,
 * the nearest neighbour with its index, a similarity transform and point-to-point ICP registration, the
 * steps of the Tanks and Temples protocol, follow, each with a host twin. Exact radius thinning, an
 * observability mask, a half-space test and masked mean / median statistics, the steps of the DTU
 * protocol, close the header, each with a host twin.
 *
 * Distance contract (bit for bit, all arithmetic fp32 and nothing contracted):
 *   - a target with a non-finite coordinate never matches; a query with one gives +inf
 *   - dx = q.x - t.x (dy, dz likewise);  d2 = (dx*dx + dy*dy) + dz*dz
 *   - m = sqrtf(min over the finite targets of d2);  result = m <= max_dist ? m : +inf
 *   - no finite target: every result is +inf
 *   - within[k] = #{i : dist_i <= tol[k]} (fp32 comparison, exact integer counts)
 *
 * Render / visibility contract (bit for bit, all arithmetic fp32, nothing contracted, every sum
 * evaluated left to right). Point i = (x, y, z) in the view of camera (K, R, t, width W, height H):
 *   - projection, the project() statement of csrc/apd_fusion.hip (ProjectCamera):
 *       tx = R0*x + R1*y + R2*z + t0;  ty = R3*x + R4*y + R5*z + t1;  tz = R6*x + R7*y + R8*z + t2
 *       d  = K6*tx + K7*ty + K8*tz
 *       px = (K0*tx + K1*ty + K2*tz) / d;  py = (K3*tx + K4*ty + K5*tz) / d
 *   - the point is dropped (takes no part in the view) if a coordinate is non-finite, or unless
 *     d > 0 and d < +inf
 *   - u = trunc_x86(px + 0.5f), v = trunc_x86(py + 0.5f): truncation, INT32_MIN for NaN and for
 *     values outside the int range (fusion's trunc_x86)
 *   - render: the point covers the pixels (a, b) with |a - u| <= splat and |b - v| <= splat that lie
 *     inside the image (no integer overflow: u = INT32_MIN covers nothing; a centre just outside
 *     still covers the part of its footprint that is inside). Every covered pixel receives the key
 *     (bits(d) << 32) | i and keeps the minimum: the nearest depth, ties to the lowest point index.
 *     depth[p] = the float in the high word, 0.0f if uncovered; index[p] = the low word, -1 if
 *     uncovered. Integer atomics: the result does not depend on the order of arrival.
 *   - visibility: point i is visible in view v iff it is not dropped, 0 <= u < W and 0 <= v < H (the
 *     centre pixel only), zb = depth_v[v*W + u] > 0, and d <= zb * (1.0f + rel_tol), the factor
 *     being one fp32 addition made once. A NaN zb compares false.
 * This is a z-buffer test; it is still not the ETH3D tool's free-space model.
 *
 * Conventions as in apd_fusion.h: plain C types, APD_OK or a negative apd_status, never exit().
 * Every data pointer (xyz, dist, tol, within, keep_idx, n_keep, the depth and index maps, seen,
 * n_visible_any) may be a host or a device pointer.
 * The calls work on the context's own stream and return after it has drained.
 *
 * These declarations are not part of apd_abi_version()'s export set (apd_hip.h + apd_fusion.h).
 */
#ifndef APD_EVAL_H_
#define APD_EVAL_H_

#include <stdint.h>
#include "apd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct apd_eval_ctx apd_eval_ctx;

apd_eval_ctx *apd_eval_create(int32_t device);
void apd_eval_destroy(apd_eval_ctx *ctx);
const char *apd_eval_last_error(const apd_eval_ctx *ctx);

/* Build the search structure over n target points (xyz interleaved, n*3 floats). Replaces any
   previous target; buffers are kept and grown, not reallocated per call.
   APD_EINVAL: n < 0, n > INT32_MAX, xyz NULL with n > 0. */
int32_t apd_eval_set_target(apd_eval_ctx *ctx, int64_t n, const float *xyz);

/* For each of n query points the truncated distance to the nearest target. dist (n floats) may be
   NULL. within (num_tol int64) may be NULL.
   APD_EINVAL: n out of range, xyz NULL with n > 0, max_dist negative or NaN (+inf: no truncation),
   num_tol < 0, tol NULL with num_tol > 0, a tol[k] negative, NaN or > max_dist.
   APD_ESTATE: no apd_eval_set_target before. */
int32_t apd_eval_distances(apd_eval_ctx *ctx, int64_t n, const float *xyz, float max_dist, float *dist,
                           int32_t num_tol, const float *tol, int64_t *within);

/* Voxel down-sampling: the voxel of a point is (floorf(x / voxel), floorf(y / voxel),
   floorf(z / voxel)) with fp32 IEEE division; points with a non-finite coordinate are dropped.
   keep_idx (room for n entries) receives the ascending indices of the lowest-index point of every
   occupied voxel, *n_keep their number.
   APD_EINVAL: n out of range, a NULL pointer with n > 0, voxel <= 0 or not finite, or an axis whose
   occupied voxel indices span more than 2^21 (the packed key has 63 bits). */
int32_t apd_eval_voxel_downsample(apd_eval_ctx *ctx, int64_t n, const float *xyz, float voxel,
                                  int32_t *keep_idx, int64_t *n_keep);

/* Device-event times of the last set_target / distances / voxel_downsample call, in ms (0 for a
   call that has not happened or launched nothing). Any pointer may be NULL. */
int32_t apd_eval_get_timing(apd_eval_ctx *ctx, double *build_ms, double *query_ms, double *voxel_ms);

/* z-buffer of a cloud in num_views cameras. cams[v].width/height give view v's size.
   depth[v]: W*H floats, 0 where nothing projects. index[v]: W*H int32, -1 there.
   index, or any index[v], may be NULL. xyz, depth[v], index[v] may be host or device
   pointers; the pointer arrays and cams are host memory. The cloud is uploaded once per call.
   The points are offered to the kernel in input order (default) or in the Morton order of the
   cloud (environment APD_EVAL_RENDER_ORDER=input|morton, read by apd_eval_create); the output does
   not depend on it.
   APD_EINVAL: n out of range, xyz NULL with n > 0, num_views < 0, cams, depth or a depth[v] NULL
   with num_views > 0, a view with width < 1, height < 1 or width*height > 2^28, splat outside 0..16. */
int32_t apd_eval_render_depth(apd_eval_ctx *ctx, int64_t n, const float *xyz, int32_t num_views,
                              const apd_camera *cams, int32_t splat,
                              float *const *depth, int32_t *const *index);

/* seen[i] = number of views in which point i is visible against depth[v] (any depth map of
   that view's size: a rendered one or a reconstructed one). n_visible_any (may be NULL) =
   #{i : seen[i] > 0}. xyz, depth[v], seen and n_visible_any may be host or device pointers.
   APD_EINVAL: as above, seen NULL with n > 0, rel_tol negative or not finite. */
int32_t apd_eval_visibility(apd_eval_ctx *ctx, int64_t n, const float *xyz, int32_t num_views,
                            const apd_camera *cams, const float *const *depth, float rel_tol,
                            int32_t *seen, int64_t *n_visible_any);

/* Device-event times of the last render_depth (sort + per view: clear, splat, resolve) and
   visibility (kernels only) call, in ms. Any pointer may be NULL. */
int32_t apd_eval_get_render_timing(apd_eval_ctx *ctx, double *render_ms, double *visibility_ms);

/* ---- scanner free-space model and voxel-averaged scores -------------------------------------------
 * Modelled on the ETH3D multi-view evaluation protocol, with this project's own exact contract (bit
 * for bit; fp32, nothing contracted, sums left to right; integer sums only, so every output is the
 * same from run to run). It differs from the ETH3D tool in known ways (a z-buffer per cube-map pixel
 * instead of per-beam cones, a free-space margin equal to the tolerance, integer-rounded voxel
 * ratios), and parity with that tool is not pinned: neither the tool nor a scan with its output is
 * at hand.
 *
 * A scanner position is the six 90-degree pinhole faces of a cube map (apd_eval_cube_cameras); the
 * scanner's own points are rendered into them with apd_eval_render_depth. A beam from the scanner to
 * one of its points proves free space along that ray, so a reconstructed point that lies in front of
 * the rendered depth by more than the tolerance is in observed free space.
 *
 * Free gap of point i against a set of views with depth maps:
 *   gap_i = max over the views v in which the point is not dropped, its centre pixel (u, v) lies
 *           inside the image and zb = depth_v[v*W + u] > 0 (a NaN zb compares false) of zb - d
 *           (one fp32 subtraction); -inf if there is no such view.
 *   Projection, drop rule and rounding are those of the visibility contract above. A +inf map entry
 *   gives +inf, equal operands give +0; no operand is NaN, so the maximum has no order.
 *
 * Voxel scores. The voxel of a point is apd_eval_voxel_downsample's; a point with a non-finite
 * coordinate belongs to no voxel and is counted nowhere. Per tolerance k and point i:
 *   good iff dist_i <= tol_k;  bad iff not good and (gap == NULL or gap_i > tol_k);  otherwise the
 *   point is unobserved. A NaN in dist or gap compares false.
 * Per voxel: a = its good points, b = its bad points; it counts for k iff a + b > 0, with the
 * integer ratio (a << 32) / (a + b) (uint64 division, rounded down).
 *   good[k], bad[k] = totals over all voxels; ratio_sum[k] = the exact integer sum of the counted
 *   voxels' ratios (< 2^63 for n <= 2^31); voxels[k] = their number.
 *   score_k = ratio_sum[k] / (voxels[k] * 2^32) in double on the host, 0 when voxels[k] is 0.
 */

/* The six faces of a cube map of size x size pixels centred at origin, in the order +X, -X, +Y, -Y,
   +Z, -Z. Rows of R (right, down, forward):
     +X (0,0,-1) (0,1,0) (1,0,0)     -X (0,0,1) (0,1,0) (-1,0,0)
     +Y (1,0,0) (0,0,-1) (0,1,0)     -Y (1,0,0) (0,0,1) (0,-1,0)
     +Z (1,0,0) (0,1,0) (0,0,1)      -Z (-1,0,0) (0,1,0) (0,0,-1)
   t = -(R origin), exact; K = [[size/2, 0, size/2 - 0.5], [0, size/2, size/2 - 0.5], [0, 0, 1]];
   width = height = size; every other field is 0. With the projection and rounding above a face
   spans exactly +-45 degrees: every direction lands in at least one face, a few on the seams in two.
   Host only: needs no context and no device.
   APD_EINVAL: size outside 2..16384, a non-finite origin, a NULL pointer. */
int32_t apd_eval_cube_cameras(const float origin[3], int32_t size, apd_camera cams[6]);

/* gap (n floats): the free gap of every point against depth[v] in cams[v]. xyz, depth[v] and gap may
   be host or device pointers; needs no apd_eval_set_target.
   APD_EINVAL: as apd_eval_visibility, with gap in place of seen. */
int32_t apd_eval_free_gap(apd_eval_ctx *ctx, int64_t n, const float *xyz, int32_t num_views,
                          const apd_camera *cams, const float *const *depth, float *gap);

/* Voxel scores of n points with their distances (and free gaps; gap may be NULL: every point that
   is not good is bad). good, bad, ratio_sum, voxels: num_tol entries each. Every data pointer may be
   a host or a device pointer; needs no apd_eval_set_target. Tolerances need not be sorted.
   APD_EINVAL: n out of range, xyz or dist NULL with n > 0, voxel <= 0 or not finite, an axis whose
   occupied voxel indices span more than 2^21, num_tol < 0, tol or an output NULL with num_tol > 0,
   a tol[k] negative or NaN. */
int32_t apd_eval_voxel_scores(apd_eval_ctx *ctx, int64_t n, const float *xyz, float voxel, const float *dist,
                              const float *gap, int32_t num_tol, const float *tol, int64_t *good, int64_t *bad,
                              uint64_t *ratio_sum, int64_t *voxels);

/* Device-event times of the last free_gap (kernels only) and voxel_scores (keys, sort, scans and
   sums) call, in ms. Any pointer may be NULL. */
int32_t apd_eval_get_protocol_timing(apd_eval_ctx *ctx, double *free_gap_ms, double *scores_ms);

/* ---- crop volume, nearest neighbour with index, registration ---------------------------------------
 * The steps the Tanks and Temples evaluation protocol adds in front of the distances: the
 * reconstruction is moved into the scan's frame by a similarity that point-to-point ICP refines, and
 * both clouds are cut to a crop volume. The contract is this project's own (bit for bit between the
 * device calls and their host twins, and the same from run to run); parity with the Tanks and Temples
 * toolbox is not pinned. Doubles throughout, nothing contracted.
 *
 * Transform. T is a 4x4 double matrix, row-major; NULL means identity. For a point (x, y, z), each
 * converted to double, row r gives
 *     p'[r] = ((T[4r]*x + T[4r+1]*y) + T[4r+2]*z) + T[4r+3]         (the last row of T is not read)
 * and q = the fp32 rounding of p' (apd_eval_transform writes q; a non-finite input gives whatever the
 * arithmetic gives).
 *
 * Crop rule (Open3D's SelectionPolygonVolume). With axis in {0, 1, 2} for X, Y, Z, (u, v, w) are the
 * coordinates (1, 2, 0), (0, 2, 1), (0, 1, 2) of p' (p' = the point itself, in double, when T is
 * NULL). The polygon is m >= 3 vertices as (U, V) double pairs. A point is kept iff its three input
 * coordinates and p' are finite, axis_min <= p'[w] <= axis_max, and the number of edges (i, (i+1) mod m)
 * with  (Vi > pv) != (Vj > pv)  and  pu < ((Uj - Ui)*(pv - Vi))/(Vj - Vi) + Ui  is odd.
 *
 * Nearest neighbour with index: apd_eval_distances' contract, plus idx[i] = the lowest index (in the
 * array given to apd_eval_set_target) among the targets that attain the minimal d2; -1 where the
 * result is +inf.
 *
 * Registration: point-to-point ICP of a source cloud against the current target. One evaluation of a
 * transform T yields 19 double sums over the source points i. q_i is the transform above; its
 * correspondence t_i is the target idx of q_i under max_dist = max_corr; it has none if that idx is
 * -1 (which includes a non-finite q_i). The terms of a point with a correspondence, coordinates
 * converted to double:
 *     [0] 1   [1..3] q   [4..6] t   [7 + 3a + b] q_a*t_b   [16] (qx*qx + qy*qy) + qz*qz
 *     [17] the fp32 minimal d2 of the distance contract, converted to double
 * and +0.0 each for a point without one; [18] is 1 for every point with a finite q_i, else +0.0.
 * Summation order: the source indices are cut into blocks of APD_EVAL_REG_BLOCK = 1024, the last one
 * padded with +0.0 terms; within a block the terms are summed by the balanced binary tree over the
 * index ((0+1)+(2+3))+...; the block sums are added left to right in block order, starting from block
 * 0's sum (no block: +0.0).
 *     n_corr = [0], n_finite = [18], fitness = n_corr / n_finite (0 if n_finite is 0),
 *     rmse = sqrt([17] / n_corr) (0 if n_corr is 0).
 * Solve (Umeyama, on the host in double): N = [0], mu_q = [1..3]/N, mu_t = [4..6]/N,
 *     C[a][b] = [7 + 3b + a]/N - mu_t[a]*mu_q[b],  var_q = [16]/N - |mu_q|^2,
 *     C = U D V^T by one-sided Jacobi rotations (the project's own 3x3 SVD, D descending),
 *     g = sign(det(U V^T)),  R = U diag(1, 1, g) V^T,  s = (D0 + D1 + g*D2)/var_q with with_scale, else 1,
 *     t = mu_t - s R mu_q,  T <- [sR | t] T.
 * Loop: evaluate T (initially T0); stop if fewer than 3 correspondences (APD_ESTATE); stop if this is
 * not the first evaluation and both |fitness - previous| < eps_fitness and |rmse - previous| <
 * eps_rmse (Open3D's rule); stop after max_iter updates; else solve, update, repeat. T is therefore
 * evaluated once more after its last update and info describes the returned T. On APD_ESTATE (fewer
 * than 3 correspondences, a covariance of rank < 2, no spread in q with with_scale) T is the last
 * transform whose evaluation had at least 3 correspondences (T0 if none) and info holds the last
 * evaluation's numbers.
 */
#define APD_EVAL_REG_BLOCK 1024

typedef struct apd_eval_reg_info {
    int32_t iterations; /* updates applied to T0 */
    int32_t reserved;
    int64_t n_corr;
    int64_t n_finite;
    double fitness;
    double rmse;
} apd_eval_reg_info;

/* keep_idx (room for n entries): the ascending indices of the kept points, *n_keep their number.
   poly: m (U, V) pairs, host memory, as are T and the scalars. xyz, keep_idx, n_keep: host or device.
   APD_EINVAL: n out of range, a NULL pointer with n > 0, n_keep or poly NULL, m < 3 or m > 2^20, a
   non-finite polygon entry, bound or entry of T, axis outside 0..2. */
int32_t apd_eval_crop_volume(apd_eval_ctx *ctx, int64_t n, const float *xyz, const double *T, int32_t axis,
                             double axis_min, double axis_max, int32_t m, const double *poly, int32_t *keep_idx,
                             int64_t *n_keep);
/* Host twin: one thread, no context, no device; every pointer is host memory. */
int32_t apd_eval_crop_volume_host(int64_t n, const float *xyz, const double *T, int32_t axis, double axis_min,
                                  double axis_max, int32_t m, const double *poly, int32_t *keep_idx, int64_t *n_keep);

/* dist (n floats) and idx (n int32) may each be NULL; host or device pointers.
   APD_EINVAL / APD_ESTATE as apd_eval_distances. */
int32_t apd_eval_nearest(apd_eval_ctx *ctx, int64_t n, const float *xyz, float max_dist, float *dist, int32_t *idx);
/* Host twin against nt target points (a uniform grid when max_dist allows one, else brute force). */
int32_t apd_eval_nearest_host(int64_t nt, const float *target, int64_t n, const float *xyz, float max_dist,
                              float *dist, int32_t *idx);

/* out (n*3 floats) = q of every point; xyz and out may be host or device pointers and may coincide.
   APD_EINVAL: n out of range, a NULL pointer with n > 0, a non-finite entry of T. */
int32_t apd_eval_transform(apd_eval_ctx *ctx, int64_t n, const float *xyz, const double *T, float *out);
int32_t apd_eval_transform_host(int64_t n, const float *xyz, const double *T, float *out);

/* T0 (may be NULL), T (16 doubles) and info are host memory; xyz is a host or a device pointer.
   APD_EINVAL: n out of range, xyz NULL with n > 0, T or info NULL, a non-finite entry of T0, max_corr
   not positive and finite, with_scale outside 0..1, max_iter outside 1..1000, an eps negative or NaN.
   APD_ESTATE: no apd_eval_set_target before, or as described above. */
int32_t apd_eval_register(apd_eval_ctx *ctx, int64_t n, const float *xyz, const double *T0, float max_corr,
                          int32_t with_scale, int32_t max_iter, double eps_fitness, double eps_rmse, double *T,
                          apd_eval_reg_info *info);
int32_t apd_eval_register_host(int64_t nt, const float *target, int64_t n, const float *xyz, const double *T0,
                               float max_corr, int32_t with_scale, int32_t max_iter, double eps_fitness,
                               double eps_rmse, double *T, apd_eval_reg_info *info);
/* The 19 sums of one evaluation of T (NULL: identity), for tests and tools. sums: host memory. */
int32_t apd_eval_register_sums(apd_eval_ctx *ctx, int64_t n, const float *xyz, const double *T, float max_corr,
                               double *sums);
int32_t apd_eval_register_sums_host(int64_t nt, const float *target, int64_t n, const float *xyz, const double *T,
                                    float max_corr, double *sums);

/* Of the last apd_eval_register / apd_eval_register_sums call: the device-event time of the fused
   evaluation kernels and of the folds (sums over the evaluations), the host time of the solves, and
   the number of evaluations. crop_ms / transform_ms: the last crop_volume / transform call's kernels.
   Any pointer may be NULL. */
int32_t apd_eval_get_register_timing(apd_eval_ctx *ctx, double *eval_ms, double *fold_ms, double *solve_ms,
                                     int32_t *evaluations, double *crop_ms, double *transform_ms);

/* ---- radius thinning, observability mask, half-space, masked statistics ------------------------------
 * The steps the DTU evaluation protocol adds around the distances: the reconstruction is thinned to a
 * minimum point spacing, accuracy counts only the points inside the scan's observability mask (a 3-D
 * byte volume), completeness only the ground-truth points above the table plane, and the scores are
 * the mean and the median of the distances below a limit. The contract is this project's own (bit for
 * bit between the device calls and their host twins, and the same from run to run); parity with the
 * DTU MATLAB code is not pinned.
 *
 * Radius thinning (the greedy maximal independent set of the radius graph, MATLAB's reducePts_haa with
 * a stated order). rank is n uint32 values, NULL meaning all equal; the priority key of point i is
 * ((uint64)rank[i] << 32) | i, lower goes first; ranks need not be distinct.
 *   - a point with a non-finite coordinate is never kept and suppresses nothing
 *   - i and j are close iff d2 <= r2, d2 = (dx*dx + dy*dy) + dz*dz the distance contract's (fp32,
 *     nothing contracted, dx = x_i - x_j), r2 = radius*radius (one fp32 product). Equality counts.
 *   - visiting the finite points in ascending key, a point is kept iff no point kept before it is
 *     close to it.
 * radius is valid iff r2 is a finite normal fp32 number (about 1.1e-19 <= radius <= 1.8e19): below
 * that the fp32 products underflow and `close` no longer bounds the coordinate differences.
 * Candidates are found in a grid of cell 2*radius, cell index floor((double)x / (2.0*radius)) per axis;
 * every decision is made by the d2 <= r2 test alone, so the grid does not enter the result. The
 * device runs the two final rules "removed once a close lower-key point is kept" and "kept once every
 * close lower-key point is removed" over a shrinking worklist until no point is undecided; that
 * fixed point is unique and equals the loop above.
 *
 * Observability mask. mask is dims[0]*dims[1]*dims[2] bytes in column-major order (MATLAB's). In
 * double: v_k = round(((double)x_k - origin[k]) / res + 1.0), C round (half away from zero).
 *   inside[i] = 1 iff the three coordinates are finite, 1 <= v_k <= dims[k] for all k and
 *   mask[(v_0 - 1) + dims[0]*((v_1 - 1) + dims[1]*(v_2 - 1))] != 0; else 0.
 *
 * Half-space. above[i] = 1 iff ((P[0]*x + P[1]*y) + P[2]*z) + P[3] > 0 in double, the coordinates
 * converted to double, nothing contracted; a NaN compares false. Else 0.
 *
 * Masked statistics of n fp32 distances. Point i is selected iff (flag == NULL or flag[i] != 0),
 * dist[i] <= limit and dist[i] < +inf (a NaN is never selected).
 *   count  = the number of selected points, exact
 *   sum    = the double sum of the selected distances, +0.0 standing for the others, in the summation
 *            order of the registration contract: blocks of APD_EVAL_REG_BLOCK indices, the balanced
 *            binary tree inside a block, the blocks left to right from block 0's sum (no block: +0.0)
 *   median = from the selected distances s in ascending order (the order of their sign-magnitude bits,
 *            so -0 < +0): odd count m: s[(m - 1)/2]; even: ((double)s[m/2 - 1] + (double)s[m/2]) / 2;
 *            m = 0: 0.
 */

/* keep_idx (room for n entries): the ascending indices of the kept points, *n_keep their number; both,
   xyz and rank may be host or device pointers.
   APD_EINVAL: n out of range, xyz, keep_idx NULL with n > 0, n_keep NULL, a radius that is not valid
   (above), an axis whose occupied cells span more than 2^21 (the packed key has 63 bits). */
int32_t apd_eval_radius_thin(apd_eval_ctx *ctx, int64_t n, const float *xyz, float radius, const uint32_t *rank,
                             int32_t *keep_idx, int64_t *n_keep);
/* Host twin: the loop itself on one thread; no context, no device; every pointer is host memory. */
int32_t apd_eval_radius_thin_host(int64_t n, const float *xyz, float radius, const uint32_t *rank, int32_t *keep_idx,
                                  int64_t *n_keep);
/* Device-event times of the last apd_eval_radius_thin call (sort_ms: bounds, keys, sort, gather and
   the neighbour runs; rounds_ms: the rounds and the final compaction) and its number of rounds. */
int32_t apd_eval_get_thin_timing(apd_eval_ctx *ctx, double *sort_ms, double *rounds_ms, int32_t *rounds);

/* rank[i] = word 0 of Philox4x32-10 with counter (i, 0, 0, 0) and key (seed, 0), the generator of the
   depth engine. Host only. APD_EINVAL: n out of range, rank NULL with n > 0. */
int32_t apd_eval_dtu_ranks(int64_t n, uint32_t seed, uint32_t *rank);

/* inside: n bytes. mask is uploaded once and kept in the context while the same pointer and dims are
   given (a caller that rewrites the array in place passes it through another call first, or destroys
   the context). xyz, mask and inside may be host or device pointers; dims and origin are host memory.
   APD_EINVAL: n out of range, a NULL pointer (xyz and inside only with n > 0), a dim < 1, a product
   of dims above 2^31, res not positive and finite, a non-finite origin. */
int32_t apd_eval_obs_mask(apd_eval_ctx *ctx, int64_t n, const float *xyz, const int32_t dims[3],
                          const double origin[3], double res, const uint8_t *mask, uint8_t *inside);
int32_t apd_eval_obs_mask_host(int64_t n, const float *xyz, const int32_t dims[3], const double origin[3], double res,
                               const uint8_t *mask, uint8_t *inside);

/* above: n bytes; xyz and above may be host or device pointers, P is host memory.
   APD_EINVAL: n out of range, P NULL, xyz or above NULL with n > 0. */
int32_t apd_eval_half_space(apd_eval_ctx *ctx, int64_t n, const float *xyz, const double P[4], uint8_t *above);
int32_t apd_eval_half_space_host(int64_t n, const float *xyz, const double P[4], uint8_t *above);

/* dist (n floats) and flag (n bytes, may be NULL) may be host or device pointers; count, sum and
   median are host memory and may each be NULL.
   APD_EINVAL: n out of range, dist NULL with n > 0, a NaN limit. */
int32_t apd_eval_masked_stats(apd_eval_ctx *ctx, int64_t n, const float *dist, const uint8_t *flag, float limit,
                              int64_t *count, double *sum, double *median);
int32_t apd_eval_masked_stats_host(int64_t n, const float *dist, const uint8_t *flag, float limit, int64_t *count,
                                   double *sum, double *median);

/* Device-event times of the last obs_mask / half_space / masked_stats call (kernels and sort, without
   the mask upload). Any pointer may be NULL. */
int32_t apd_eval_get_dtu_timing(apd_eval_ctx *ctx, double *mask_ms, double *half_space_ms, double *stats_ms);

#ifdef __cplusplus
}
#endif

#endif /* APD_EVAL_H_ */
