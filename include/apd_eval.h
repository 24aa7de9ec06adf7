/*
 * apd_eval.h — C-ABI of the device-side point-cloud evaluation (libapd_hip.so).
 *
 * The reference hands accuracy / completeness / F1 to an external evaluator binary
 * (tools/eval_eth_train.py). This ABI computes the part of that which is heavy: for every point of
 * one cloud the distance to the nearest point of another, truncated at max_dist, plus a voxel
 * down-sampling of a cloud. It is the plain nearest-neighbour definition (DTU-style); the ETH3D
 * tool's free-space and visibility handling is not modelled. A z-buffer renderer of a cloud into
 * cameras and a per-point visibility count against depth maps serve a plain visibility filter.
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

#ifdef __cplusplus
}
#endif

#endif /* APD_EVAL_H_ */
