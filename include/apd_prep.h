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
 * Undistortion (apd_prepare --undistort). An image taken with one of COLMAP's distorted camera
 * models is warped into the image of a pinhole camera. Model ids and parameter orders are COLMAP's:
 *      0 SIMPLE_PINHOLE         f cx cy                    1 PINHOLE        fx fy cx cy
 *      2 SIMPLE_RADIAL          f cx cy k                  3 RADIAL         f cx cy k1 k2
 *      4 OPENCV                 fx fy cx cy k1 k2 p1 p2    5 OPENCV_FISHEYE fx fy cx cy k1 k2 k3 k4
 *      6 FULL_OPENCV            fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
 *      8 SIMPLE_RADIAL_FISHEYE  f cx cy k                  9 RADIAL_FISHEYE f cx cy k1 k2
 *     10 THIN_PRISM_FISHEYE     fx fy cx cy k1 k2 p1 p2 k3 k4 sx1 sy1
 * 0 and 1 are the identity distortion; FOV (7) is not supported. For the f models fx = fy = f.
 *
 * Forward function, normalised pinhole (u, v) -> normalised distorted (ud, vd), r2 = u*u + v*v:
 *     SIMPLE_RADIAL  rad = k*r2;                 ud = u + u*rad;  vd = v + v*rad
 *     RADIAL         rad = k1*r2 + (k2*r2)*r2;   as SIMPLE_RADIAL
 *     OPENCV         rad as RADIAL
 *                    ud = u + ((u*rad + ((2*p1)*u)*v) + p2*(r2 + (2*u)*u))
 *                    vd = v + ((v*rad + ((2*p2)*u)*v) + p1*(r2 + (2*v)*v))
 *     FULL_OPENCV    g = (1 + r2*(k1 + r2*(k2 + r2*k3))) / (1 + r2*(k4 + r2*(k5 + r2*k6)))
 *                    ud = (u*g + ((2*p1)*u)*v) + p2*(r2 + (2*u)*u)
 *                    vd = (v*g + ((2*p2)*u)*v) + p1*(r2 + (2*v)*v)
 *     fisheye family r = sqrt(r2); s = 1 if r2 == 0 else atan_c(r)/r; a = u*s; b = v*s; t2 = a*a + b*b
 *       SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE: their radial term on (a, b) with t2 for r2
 *       OPENCV_FISHEYE      rad = t2*(k1 + t2*(k2 + t2*(k3 + t2*k4)));  ud = a + a*rad;  vd = b + b*rad
 *       THIN_PRISM_FISHEYE  the same rad
 *                    ud = a + (((a*rad + ((2*p1)*a)*b) + p2*(t2 + (2*a)*a)) + sx1*t2)
 *                    vd = b + (((b*rad + ((2*p2)*a)*b) + p1*(t2 + (2*b)*b)) + sy1*t2)
 *
 * atan_c(x), x >= 0, with + - * / and comparisons only (no libm, so host, device and a restatement
 * agree to the bit); it is fdlibm's reduction and polynomial:
 *     x >= 2^66:   hi3 + lo3                       x < 2^-29:  x
 *     x < 7/16:    t = x, no reduction             x < 11/16:  t = (2*x - 1)/(2 + x), hi0, lo0
 *     x < 19/16:   t = (x - 1)/(x + 1), hi1, lo1   x < 39/16:  t = (x - 1.5)/(1 + 1.5*x), hi2, lo2
 *     else:        t = -1/x, hi3, lo3
 *     z = t*t; w = z*z
 *     s1 = z*(A0 + w*(A2 + w*(A4 + w*(A6 + w*(A8 + w*A10)))))
 *     s2 = w*(A1 + w*(A3 + w*(A5 + w*(A7 + w*A9))))
 *     no reduction: t - t*(s1 + s2);  else: hi - ((t*(s1 + s2) - lo) - t)
 *     hi0..3 = 4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
 *              1.57079632679489655800e+00
 *     lo0..3 = 2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
 *              6.12323399573676603587e-17
 *     A0..10 = 3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
 *              -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
 *              6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
 *              -3.65315727442169155270e-02, 1.62858201153657823623e-02
 *
 * Warp. Source and destination are 8-bit BGR, interleaved, row-major. For output pixel (x, y), with
 * the output camera out_K = {out_fx, out_fy, out_cx, out_cy} and the source camera's fx fy cx cy:
 *     u = ((x + 0.5) - out_cx)/out_fx;  v = ((y + 0.5) - out_cy)/out_fy       (pixel centres at .5)
 *     (ud, vd) = forward(u, v);  sx = (fx*ud + cx) - 0.5;  sy = (fy*vd + cy) - 0.5
 *     if !(sx > -1 && sx < src_w && sy > -1 && sy < src_h): the pixel is 0 0 0 (a NaN fails the test)
 *     ix = floor(sx); wx = (int)floor((sx - ix)*256 + 0.5) in 0..256; iy, wy likewise
 *     channel = (T00*(256-wx)*(256-wy) + T10*wx*(256-wy) + T01*(256-wx)*wy + T11*wx*wy + 32768) >> 16
 * in integers, where Tab is the source at (ix + a, iy + b) and a tap outside the image is 0: bilinear
 * with weights of 1/256 and a black border, so that regions without a source are visibly blank.
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

/* The warp of the contract's "Undistortion" section on the device. params: the n_params parameters
   of model_id (host memory); src: src_w*src_h*3 bytes, dst: out_w*out_h*3 bytes, host or device
   pointers; out_K: {fx, fy, cx, cy} of the output camera (host memory). Needs no model.
   APD_EINVAL: an unknown or unsupported model id (FOV included), n_params not the model's count, a
   non-finite parameter or out_K entry, a focal length (source or output) that is not positive, a
   size outside 1..65536, a NULL pointer. APD_ENOMEM as elsewhere. */
int32_t apd_prep_undistort_bgr8(apd_prep_ctx *ctx, int32_t model_id, const double *params, int32_t n_params,
                                int32_t src_w, int32_t src_h, const uint8_t *src, const double *out_K, int32_t out_w,
                                int32_t out_h, uint8_t *dst);

/* Device-event times in ms of the last apd_prep_undistort_bgr8: the copy of the source into the
   context's buffer, the kernel, the copy of the result out of it. Any pointer may be NULL. */
int32_t apd_prep_get_undistort_timing(apd_prep_ctx *ctx, double *upload_ms, double *kernel_ms, double *download_ms);

/* Host only, like apd_prep_cos_gate: no context, no device.
   apd_prep_undistort_bgr8_host: the same warp on the CPU (one thread), host pointers, same errors.
   apd_prep_atan_c: the contract's atan_c.
   apd_prep_undistort_xy: n distorted pixel coordinates (x, y pairs, COLMAP's convention: the centre of
   the top-left pixel is (0.5, 0.5)) -> the coordinates in the pinhole camera with the same fx fy cx cy.
   With t = ((x - cx)/fx, (y - cy)/fy), Newton's method on forward(p) - t from p = t; the Jacobian
   from central differences of step 1e-6; at most 100 steps, stopping when both components of a step
   are below 1e-10; the result is (fx*u + cx, fy*v + cy). A point that does not get there or leaves
   the finite numbers is written as (-1, -1) and counted in *unresolved (may be NULL). xy_in and
   xy_out may be the same array. APD_EINVAL: model or parameters as above, n < 0, a NULL array with
   n > 0. */
int32_t apd_prep_undistort_bgr8_host(int32_t model_id, const double *params, int32_t n_params, int32_t src_w,
                                     int32_t src_h, const uint8_t *src, const double *out_K, int32_t out_w,
                                     int32_t out_h, uint8_t *dst);
double apd_prep_atan_c(double x);
int32_t apd_prep_undistort_xy(int32_t model_id, const double *params, int32_t n_params, int64_t n, const double *xy_in,
                              double *xy_out, int64_t *unresolved);

#ifdef __cplusplus
}
#endif

#endif /* APD_PREP_H_ */
