/*
 * apd_eval.h — C-ABI of the device-side point-cloud evaluation (libapd_hip.so).
 *
 * The reference hands accuracy / completeness / F1 to an external evaluator binary
 * (tools/eval_eth_train.py). This ABI computes the part of that which is heavy: for every point of
 * one cloud the distance to the nearest point of another, truncated at max_dist, plus a voxel
 * down-sampling of a cloud. It is the plain nearest-neighbour definition (DTU-style); the ETH3D
 * tool's free-space and visibility handling is not modelled.
 *
 * Distance contract (bit for bit, all arithmetic fp32 and nothing contracted):
 *   - a target with a non-finite coordinate never matches; a query with one gives +inf
 *   - dx = q.x - t.x (dy, dz likewise);  d2 = (dx*dx + dy*dy) + dz*dz
 *   - m = sqrtf(min over the finite targets of d2);  result = m <= max_dist ? m : +inf
 *   - no finite target: every result is +inf
 *   - within[k] = #{i : dist_i <= tol[k]} (fp32 comparison, exact integer counts)
 *
 * Conventions as in apd_fusion.h: plain C types, APD_OK or a negative apd_status, never exit().
 * Every data pointer (xyz, dist, tol, within, keep_idx, n_keep) may be a host or a device pointer.
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

#ifdef __cplusplus
}
#endif

#endif /* APD_EVAL_H_ */
