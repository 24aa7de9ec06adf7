/*
 * apd_prep.h — C-ABI of the device side of scan preparation (libapd_hip.so).
 *
 * The reference turns a COLMAP sparse model into a scan (cams/, images/, pair.txt) with
 * tools/colmap2mvsnet.py. Two parts of that are heavy: the covisibility score of every image pair
 * (calc_score, :316-340, :470-487) and the per-image depth range (:415-431). This ABI computes the
 * integer counts the score is made of and the order statistics the depth range is made of; the score,
 * the selection and every file are the host's (host/prepare_main.cpp, apd_abi.prepare_views).
 *
 * Contract (bit for bit). All arithmetic is IEEE double with nothing contracted, every sum is
 * evaluated left to right as written, every accumulation is an integer.
 *
 * Model. Images are numbered 0..n-1 in ascending COLMAP image id (:399-402). From the quaternion
 * (w, x, y, z), not normalised, by qvec2rotmat (:289-299) with squares written as products:
 *     R = [[(1 - 2*(y*y)) - 2*(z*z), (2*x)*y - (2*w)*z,       (2*z)*x + (2*w)*y      ],
 *          [(2*x)*y + (2*w)*z,       (1 - 2*(x*x)) - 2*(z*z), (2*y)*z - (2*w)*x      ],
 *          [(2*z)*x - (2*w)*y,       (2*y)*z + (2*w)*x,       (1 - 2*(x*x)) - 2*(y*y)]]
 *     centre c_k = -((R[0][k]*t0 + R[1][k]*t1) + R[2][k]*t2)
 * An observation is an (image, point) entry of an image's 2D-point list whose point id is not -1.
 * R, t and the centres are computed by the caller (the host) and handed over; points are handed
 * over as an array and observations refer to it by index, grouped by image (CSR).
 *
 * Pair counts. Observations of the same point in the same image collapse to one (the reference
 * counts an image's duplicates once per duplicate, from the lower-numbered image only). For every
 * point, every unordered pair a < b of distinct images that observe it is one record; with the
 * point p and the centres ca, cb:
 *     u = ca - p;  v = cb - p
 *     q = (((u0*v0 + u1*v1) + u2*v2) / sqrt((u0*u0 + u1*u1) + u2*u2)) / sqrt((v0*v0 + v1*v1) + v2*v2)
 * shared[a][b] = the records of the pair; narrow[a][b] = those with q >= q_gate (a NaN q, a point at
 * a camera centre, compares false; a q above 1 from rounding counts). Both are symmetric n x n
 * uint32 matrices with zero diagonals.
 *
 * Score (host): score = shared, except score = 0 where narrow >= floor(3*shared/4) + 1. That is the
 * reference's "the element of rank int(len*0.75) of the ascending angles is < 1 degree" without a
 * sort, with q_gate = apd_prep_cos_gate(1.0).
 *
 * Depth ranks. Per image i, zc = ((R[2][0]*x + R[2][1]*y) + R[2][2]*z) + t2 over all n_i of its
 * observations (duplicates and points behind the camera included), sorted ascending (by the total
 * order of the bit patterns: -0 before +0). z_at[i][k] = the element at index
 * min((int64)((double)n_i * f_k), n_i - 1) for fractions 0 <= f_k < 1. A row with n_i = 0 carries
 * no entry (it is filled with 0).
 *
 * No float atomics: every output is the same from run to run and under any permutation of the
 * points, of the observations within an image and of the images' order of arrival.
 *
 * Conventions as in apd_eval.h: plain C types, APD_OK or a negative apd_status, never exit(); the
 * calls work on the context's own stream and return after it has drained; buffers are kept and
 * grown. The inputs of apd_prep_set_model are host memory (they are validated on the host);
 * shared, narrow, z_at and fractions may be host or device pointers.
 *
 * These declarations are not part of apd_abi_version()'s export set.
 */
#ifndef APD_PREP_H_
#define APD_PREP_H_

#include <stdint.h>
#include "apd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define APD_PREP_MAX_IMAGES 16384

typedef struct apd_prep_ctx apd_prep_ctx;

apd_prep_ctx *apd_prep_create(int32_t device);
void apd_prep_destroy(apd_prep_ctx *ctx);
const char *apd_prep_last_error(const apd_prep_ctx *ctx);

/* The model: rot n_images*9 (row-major R), trans n_images*3, centres n_images*3, xyz n_points*3
   doubles; obs_offset n_images+1 ascending int64 with obs_offset[0] = 0 and obs_offset[n_images] =
   n_obs; obs_point[obs_offset[i] .. obs_offset[i+1]) = the point indices image i observes, in any
   order, duplicates allowed. Uploads the model and builds the tracks (sorted, duplicate-free
   (point, image) keys, per-point lengths L and the exclusive scan of L(L-1)/2 as uint64). Replaces
   any previous model.
   APD_EINVAL: n_images outside 1..APD_PREP_MAX_IMAGES, n_points or n_obs negative or above
   INT32_MAX, a NULL pointer with a non-zero count, offsets that do not ascend from 0 to n_obs, a
   point index outside 0..n_points-1, a non-finite double. */
int32_t apd_prep_set_model(apd_prep_ctx *ctx, int32_t n_images, const double *rot, const double *trans,
                           const double *centres, int64_t n_points, const double *xyz, int64_t n_obs,
                           const int64_t *obs_offset, const int32_t *obs_point);

/* How the pair records reach the matrices: per-workgroup aggregation in LDS before the global
   atomics, or every record straight to a global atomic. The result is the same. DEFAULT picks the
   LDS path when there are at least 32 records per image pair on average, else the global one. */
#define APD_PREP_ATOMICS_DEFAULT 0
#define APD_PREP_ATOMICS_GLOBAL 1
#define APD_PREP_ATOMICS_LDS 2

/* shared, narrow: n_images*n_images uint32 each (narrow may be NULL). *n_records (may be NULL) =
   the number of pair records, the sum over tracks of L(L-1)/2.
   APD_EINVAL: shared NULL, q_gate NaN, atomics not one of the three. APD_ESTATE: no model. */
int32_t apd_prep_pair_counts(apd_prep_ctx *ctx, double q_gate, int32_t atomics, uint32_t *shared, uint32_t *narrow,
                             uint64_t *n_records);

/* z_at: n_images*num_fractions doubles, row i for image i. n_obs_out (may be NULL): n_images int64.
   APD_EINVAL: num_fractions outside 1..64, a NULL fractions or z_at, a fraction outside [0, 1) or NaN
   (fractions are read on the host if they are host memory, else copied back first).
   APD_ESTATE: no model. */
int32_t apd_prep_depth_ranks(apd_prep_ctx *ctx, int32_t num_fractions, const double *fractions, double *z_at,
                             int64_t *n_obs_out);

/* Device-event times in ms of the last set_model (tracks: keys, sort, heads, scans), pair_counts
   (pairs: clear, records, mirror; records: the record kernel alone) and depth_ranks (z, segmented
   sort, pick). Any pointer may be NULL. */
int32_t apd_prep_get_timing(apd_prep_ctx *ctx, double *tracks_ms, double *pairs_ms, double *records_ms,
                            double *ranks_ms);

/* The smallest double q with (180/pi)*acos(q) < degrees, by bisection with libm acos (as fusion's
   angle_cut_lt does for floats); monotonicity is checked for 64 doubles on either side of the cut.
   Host only: needs no context and no device. NaN if degrees is not in (0, 180] or the check fails. */
double apd_prep_cos_gate(double degrees);

#ifdef __cplusplus
}
#endif

#endif /* APD_PREP_H_ */
