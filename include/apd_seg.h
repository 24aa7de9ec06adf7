/*
 * apd_seg.h — C-ABI of flat-zone sa_masks (libapd_hip.so): the mask step of the workflow
 * apd_prepare -> apd_segment (optional) -> apd -> apd_eval.
 *
 * The reference makes sa_masks/<view>.bin with tools/run_SAM.py, a learned model (SAM, ViT-H). This is
 * NOT that model and makes no such masks. It labels flat zones: the 4-connected regions in which the
 * smoothed image varies slowly. The engine needs a uint8 label per pixel, 0 = "no prior here", k > 0 =
 * "use only taps and anchors that carry my label"; textured pixels and edges keep 0, which is exactly
 * "run this pixel as without SA". Whether such masks help a reconstruction is not measured.
 *
 * Contract (bit for bit). All arithmetic is integer; no result depends on thread order. The input is
 * 8-bit BGR, interleaved, row-major, w x h. / is integer division of non-negative numbers.
 *
 * 1. Downscale. s = 1 if max_size == 0 or max(w, h) <= max_size, else s = ceil(max(w, h) / max_size).
 *    Working size W = ceil(w / s), H = ceil(h / s). Working pixel (X, Y), channel c:
 *        sum = the sum of the source's channel c over x in [X*s, min(w, (X+1)*s)), y in [Y*s, min(h, (Y+1)*s))
 *        cnt = the number of those pixels (partial blocks at the right and bottom use their own)
 *        I_c(X, Y) = (2*sum + cnt) / (2*cnt)                                  the mean, rounded half up
 *    With s = 1 the working image is the source. Masks are written at the working size; `apd` resizes a
 *    mask of another size with INTER_NEAREST.
 *
 * 2. Smooth. The separable binomial filter 1 4 6 4 1, horizontally then vertically, coordinates
 *    clamped to the image, never rounded:
 *        T_c(x, y) = I_c(x-2, y) + 4*I_c(x-1, y) + 6*I_c(x, y) + 4*I_c(x+1, y) + I_c(x+2, y)
 *        S_c(x, y) = T_c(x, y-2) + 4*T_c(x, y-1) + 6*T_c(x, y) + 4*T_c(x, y+1) + T_c(x, y+2)
 *    S_c is a uint16, 256 x the smoothed grey level, at most 65280.
 *
 * 3. Flatness. d(p, q) = max over c of |S_c(p) - S_c(q)|; g(p) = the maximum of d(p, q) over the up to
 *    eight neighbours q of p inside the image (0 if there is none); flat(p) = g(p) <= threshold_q8, an
 *    integer in units of 1/256 grey level.
 *
 * 4. Components. The 4-connected components of the flat pixels. A component's root is the smallest
 *    linear index y*W + x among its pixels. (Two flat 4-neighbours differ by at most the threshold,
 *    so there is no separate link test.)
 *
 * 5. Areas and ranking. A component's area is its pixel count. Components with area < min_area are
 *    dropped. The survivors are ordered by area descending, ties by root ascending; the first 255 get
 *    the labels 1..255. Every other pixel gets 0: non-flat pixels, pixels of dropped components and
 *    pixels of survivors beyond the 255th.
 *
 * Outputs: the W x H uint8 label map, n_survivors (before the cap), n_labels = min(n_survivors, 255).
 *
 * Picture (apd_segment's sa_masks/<view>.png): label 0 is white (255, 255, 255); label k > 0 is
 *     B = (37*k + 11) % 224,  G = (91*k + 53) % 224,  R = (151*k + 101) % 224
 * (apd_seg_label_colour), never white; a pure function of k where the reference's script draws random
 * colours.
 *
 * Conventions as in apd_prep.h: plain C types, APD_OK or a negative apd_status, never exit(); the
 * calls work on the context's own stream and return after it has drained; buffers are kept and
 * grown. Images, masks, label maps and stage outputs may be host or device pointers.
 *
 * These declarations are not part of apd_abi_version()'s export set.
 */
#ifndef APD_SEG_H_
#define APD_SEG_H_

#include <stdint.h>
#include "apd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define APD_SEG_MAX_SIDE 65536
#define APD_SEG_MAX_THRESHOLD_Q8 65280
#define APD_SEG_MAX_LABELS 255

typedef struct apd_seg_ctx apd_seg_ctx;

apd_seg_ctx *apd_seg_create(int32_t device);
void apd_seg_destroy(apd_seg_ctx *ctx);
const char *apd_seg_last_error(const apd_seg_ctx *ctx);

/* Stages 1 to 5. src: w*h*3 bytes; labels: W*H bytes, W = *out_w, H = *out_h (apd_seg_working_size
   gives them beforehand). n_survivors and n_labels may be NULL.
   APD_EINVAL: w or h outside 1..APD_SEG_MAX_SIDE, W*H above INT32_MAX, max_size < 0, threshold_q8
   outside 0..APD_SEG_MAX_THRESHOLD_Q8, min_area < 1, a NULL src, labels, out_w or out_h. */
int32_t apd_seg_flat_zones_bgr8(apd_seg_ctx *ctx, int32_t w, int32_t h, const uint8_t *src, int32_t max_size,
                                int32_t threshold_q8, int32_t min_area, uint8_t *labels, int32_t *out_w,
                                int32_t *out_h, int32_t *n_survivors, int32_t *n_labels);

/* Stage 4 alone on the caller's mask (W*H bytes, non-zero = set): roots[i] = the root of pixel i's
   component, -1 where the mask is 0.
   APD_EINVAL: W or H outside 1..APD_SEG_MAX_SIDE, W*H above INT32_MAX, a NULL pointer. */
int32_t apd_seg_label_mask(apd_seg_ctx *ctx, int32_t W, int32_t H, const uint8_t *mask_u8, int32_t *roots_i32);

/* Intermediate results of the context's last successful call, at the working size W x H:
     WORK    W*H*3 uint8   the working image, interleaved BGR
     SMOOTH  3*W*H uint16  the planes S_0 (B), S_1, S_2, one after the other
     FLAT    W*H uint8     1 where flat, else 0 (after apd_seg_label_mask: the caller's mask)
     ROOTS   W*H int32     the root of the pixel's component, -1 where not flat
     AREAS   W*H int32     at a root's index its component's area, 0 elsewhere
   APD_EINVAL: an unknown stage, a NULL out. APD_ESTATE: no call yet, or WORK or SMOOTH after
   apd_seg_label_mask, which has neither. */
#define APD_SEG_STAGE_WORK 0
#define APD_SEG_STAGE_SMOOTH 1
#define APD_SEG_STAGE_FLAT 2
#define APD_SEG_STAGE_ROOTS 3
#define APD_SEG_STAGE_AREAS 4
int32_t apd_seg_get_stage(apd_seg_ctx *ctx, int32_t which, void *out);

/* Device-event times in ms of the last call, ms[APD_SEG_NUM_TIMES]: the copy of the input into the
   context, the kernels of each stage (0 for one that did not run), the ranking (compaction, sort, the
   read-back of at most 255 survivors, the table) and the copy of the result out of the context. */
#define APD_SEG_T_UPLOAD 0
#define APD_SEG_T_DOWNSCALE 1
#define APD_SEG_T_SMOOTH_FLAT 2
#define APD_SEG_T_CCL_TILE 3
#define APD_SEG_T_CCL_MERGE 4
#define APD_SEG_T_FLATTEN_AREA 5
#define APD_SEG_T_RANK 6
#define APD_SEG_T_RELABEL 7
#define APD_SEG_T_DOWNLOAD 8
#define APD_SEG_NUM_TIMES 9
int32_t apd_seg_get_timing(apd_seg_ctx *ctx, double *ms);

/* Host only: no context, no device, one thread, host pointers; the same results bit for bit and the
   same errors. apd_seg_flat_zones_bgr8_host has the device call's outputs plus, each optional (NULL)
   and of the size apd_seg_get_stage states: work, smooth, flat, roots, areas.
   apd_seg_working_size: s, W, H of stage 1 (any pointer may be NULL); APD_EINVAL as above.
   apd_seg_label_colour: the picture's colour of label k (0..255) as B, G, R. */
int32_t apd_seg_flat_zones_bgr8_host(int32_t w, int32_t h, const uint8_t *src, int32_t max_size, int32_t threshold_q8,
                                     int32_t min_area, uint8_t *labels, int32_t *out_w, int32_t *out_h,
                                     int32_t *n_survivors, int32_t *n_labels, uint8_t *work, uint16_t *smooth,
                                     uint8_t *flat, int32_t *roots, int32_t *areas);
int32_t apd_seg_label_mask_host(int32_t W, int32_t H, const uint8_t *mask_u8, int32_t *roots_i32);
int32_t apd_seg_working_size(int32_t w, int32_t h, int32_t max_size, int32_t *s, int32_t *W, int32_t *H);
void apd_seg_label_colour(int32_t k, uint8_t bgr[3]);

#ifdef __cplusplus
}
#endif

#endif /* APD_SEG_H_ */
