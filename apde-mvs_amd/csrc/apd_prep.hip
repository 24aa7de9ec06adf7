// apd_prep.hip — device side of scan preparation (include/apd_prep.h): pair counts by tracks and
// per-image depth order statistics. gfx950; double arithmetic, nothing contracted (-ffp-contract=off),
// integer atomics only.
//
// Tracks:       k_pr_keys -> rocprim radix sort -> k_pr_heads -> two exclusive scans -> k_pr_tracks
//               -> k_pr_track_records -> exclusive scan (uint64)
// Pair records: k_pr_pairs<AGG>: the records are dealt over lanes in runs of ITEMS consecutive
//               records; a run finds its track by binary search in the scan, unranks the triangular
//               index once and then steps (a, b) forward. AGG: the records of a workgroup's tile are
//               summed in an LDS hash table keyed by (a, b) before one global atomic per distinct pair.
// Depth ranks:  k_pr_depth_keys -> rocprim segmented radix sort -> k_pr_pick
// Undistortion: k_pr_undistort<MODEL>: one output pixel per lane in 64 x 4 tiles, the arithmetic of
//               apd_undistort.h; the camera travels in the kernel arguments.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/apd_prep.h"
#include "apd_host.h"
#include "apd_undistort.h"

namespace {

constexpr int BLOCK = 256;
constexpr int ITEMS = 8;               // consecutive records per lane
constexpr int TILE = BLOCK * ITEMS;    // records per workgroup pass
constexpr int SLOTS = 4096;            // LDS table entries (key + two counts = 48 KiB)
constexpr int PROBES = 16;             // linear probes before a record goes straight to global memory
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr int PAIR_GRID = 8192;

// the image of observation j: the last i with off[i] <= j (off has n + 1 entries, off[n] > j)
__device__ __forceinline__ int image_of(const int64_t *__restrict__ off, int n, int64_t j) {
    int lo = 0, hi = n;  // invariant: off[lo] <= j < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(BLOCK) k_pr_keys(const int64_t *__restrict__ off, int n_images,
                                                   const int *__restrict__ obs_point, int n_obs, uint64_t *keys) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_obs) return;
    keys[j] = ((uint64_t)(uint32_t)obs_point[j] << 32) | (uint32_t)image_of(off, n_images, j);
}

// head_u: first of a run of equal (point, image) keys; head_p: first key of a point
__global__ void __launch_bounds__(BLOCK) k_pr_heads(const uint64_t *__restrict__ keys, int n_obs, uint32_t *head_u,
                                                    uint32_t *head_p) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_obs) return;
    const uint64_t k = keys[j];
    const uint64_t p = j ? keys[j - 1] : 0;
    head_u[j] = (j == 0 || k != p) ? 1u : 0u;
    head_p[j] = (j == 0 || (k >> 32) != (p >> 32)) ? 1u : 0u;
}

// u_image[pos_u]: the image of every distinct key; t_start[pos_p] / t_point[pos_p]: where a point's
// distinct keys start and which point it is. counts[0] = distinct keys, counts[1] = tracks; the
// last lane also closes t_start.
__global__ void __launch_bounds__(BLOCK) k_pr_tracks(const uint64_t *__restrict__ keys, int n_obs,
                                                     const uint32_t *__restrict__ head_u,
                                                     const uint32_t *__restrict__ head_p,
                                                     const uint32_t *__restrict__ pos_u,
                                                     const uint32_t *__restrict__ pos_p, uint32_t *u_image,
                                                     uint32_t *t_start, uint32_t *t_point, uint32_t *counts) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_obs) return;
    const uint64_t k = keys[j];
    const uint32_t hu = head_u[j], hp = head_p[j], pu = pos_u[j], pp = pos_p[j];
    if (hu) u_image[pu] = (uint32_t)k;
    if (hp) {
        t_start[pp] = pu;
        t_point[pp] = (uint32_t)(k >> 32);
    }
    if (j == n_obs - 1) {
        counts[0] = pu + hu;
        counts[1] = pp + hp;
        t_start[pp + hp] = pu + hu;
    }
}

// rec[t] = L(L-1)/2 for t < n_tracks, rec[n_tracks] = 0 (the scan's last entry is then the total)
__global__ void __launch_bounds__(BLOCK) k_pr_track_records(const uint32_t *__restrict__ t_start, int n_tracks,
                                                            uint64_t *rec) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t > n_tracks) return;
    uint64_t r = 0;
    if (t < n_tracks) {
        const uint64_t L = t_start[t + 1] - t_start[t];
        r = L * (L - 1) / 2;
    }
    rec[t] = r;
}

// first record of row a in a track of length L: a rows of (L-1), (L-2), ... entries
__device__ __forceinline__ uint64_t row_start(uint64_t a, uint64_t L) { return a * (2 * L - a - 1) / 2; }

// k in [0, L(L-1)/2) -> (a, b), a < b < L, rows first. The square root gives a guess; the integer
// steps make it exact whatever the root's rounding.
__device__ __forceinline__ void unrank(uint64_t k, uint32_t L, uint32_t &a, uint32_t &b) {
    const double m = 2.0 * (double)L - 1.0;
    double root = m * m - 8.0 * (double)k;
    root = root > 0.0 ? sqrt(root) : 0.0;
    int64_t g = (int64_t)((m - root) * 0.5);
    if (g < 0) g = 0;
    if (g > (int64_t)L - 2) g = (int64_t)L - 2;
    while (g > 0 && row_start((uint64_t)g, L) > k) --g;
    while (g < (int64_t)L - 2 && row_start((uint64_t)g + 1, L) <= k) ++g;
    a = (uint32_t)g;
    b = (uint32_t)(g + 1 + (int64_t)(k - row_start((uint64_t)g, L)));
}

struct PairArgs {
    const uint64_t *rec_off;   // n_tracks + 1, exclusive scan of the records per track
    const uint32_t *t_start;   // n_tracks + 1
    const uint32_t *t_point;   // n_tracks
    const uint32_t *u_image;   // distinct keys
    const double *centres;     // n_images * 3
    const double *xyz;         // n_points * 3
    uint32_t *shared, *narrow; // n_images * n_images
    uint64_t total;
    double q_gate;
    int n_tracks, n_images;
};

__device__ __forceinline__ bool is_narrow(const double *__restrict__ ca, const double *__restrict__ cb, double px,
                                          double py, double pz, double q_gate) {
    const double u0 = ca[0] - px, u1 = ca[1] - py, u2 = ca[2] - pz;
    const double v0 = cb[0] - px, v1 = cb[1] - py, v2 = cb[2] - pz;
    const double q = (((u0 * v0 + u1 * v1) + u2 * v2) / sqrt((u0 * u0 + u1 * u1) + u2 * u2)) /
                     sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    return q >= q_gate;
}

template <bool AGG>
__global__ void __launch_bounds__(BLOCK) k_pr_pairs(const PairArgs A) {
    __shared__ uint32_t s_key[AGG ? SLOTS : 1];
    __shared__ uint32_t s_shared[AGG ? SLOTS : 1];
    __shared__ uint32_t s_narrow[AGG ? SLOTS : 1];
    const uint64_t tiles = (A.total + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (AGG) {
            for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
                s_key[s] = EMPTY;
                s_shared[s] = 0;
                s_narrow[s] = 0;
            }
            __syncthreads();
        }
        uint64_t r = tile * TILE + (uint64_t)threadIdx.x * ITEMS;
        const uint64_t r_end = r + ITEMS < A.total ? r + ITEMS : A.total;
        if (r < r_end) {
            int lo = 0, hi = A.n_tracks;  // rec_off[lo] <= r < rec_off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (A.rec_off[mid] <= r) lo = mid; else hi = mid;
            }
            int t = lo;
            uint32_t base = A.t_start[t], L = A.t_start[t + 1] - base, a, b;
            unrank(r - A.rec_off[t], L, a, b);
            uint32_t pt = A.t_point[t];
            double px = A.xyz[3 * (size_t)pt], py = A.xyz[3 * (size_t)pt + 1], pz = A.xyz[3 * (size_t)pt + 2];
            uint32_t ia = A.u_image[base + a];
            for (;;) {
                const uint32_t ib = A.u_image[base + b];
                const bool nar = is_narrow(A.centres + 3 * (size_t)ia, A.centres + 3 * (size_t)ib, px, py, pz, A.q_gate);
                const uint32_t key = ia * (uint32_t)A.n_images + ib;  // < 2^28
                bool done = false;
                if (AGG) {
                    uint32_t s = (key * 2654435761u) >> 20;  // 12 bits = SLOTS
                    for (int probe = 0; probe < PROBES; ++probe) {
                        const uint32_t old = atomicCAS(&s_key[s], EMPTY, key);
                        if (old == EMPTY || old == key) {
                            atomicAdd(&s_shared[s], 1u);
                            if (nar) atomicAdd(&s_narrow[s], 1u);
                            done = true;
                            break;
                        }
                        s = (s + 1) & (SLOTS - 1);
                    }
                }
                if (!done) {
                    atomicAdd(&A.shared[key], 1u);
                    if (nar) atomicAdd(&A.narrow[key], 1u);
                }
                if (++r >= r_end) break;
                if (++b == L) {
                    if (++a == L - 1) {  // next track that has records (one exists: r < total)
                        do {
                            ++t;
                            base = A.t_start[t];
                            L = A.t_start[t + 1] - base;
                        } while (L < 2);
                        a = 0;
                        pt = A.t_point[t];
                        px = A.xyz[3 * (size_t)pt];
                        py = A.xyz[3 * (size_t)pt + 1];
                        pz = A.xyz[3 * (size_t)pt + 2];
                    }
                    b = a + 1;
                    ia = A.u_image[base + a];
                }
            }
        }
        if (AGG) {
            __syncthreads();
            for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
                const uint32_t key = s_key[s];
                if (key != EMPTY) {
                    atomicAdd(&A.shared[key], s_shared[s]);
                    if (s_narrow[s]) atomicAdd(&A.narrow[key], s_narrow[s]);
                }
            }
            __syncthreads();
        }
    }
}

// the records fill the upper triangle (a < b); copy it below the diagonal
__global__ void __launch_bounds__(BLOCK) k_pr_mirror(uint32_t *m0, uint32_t *m1, int n) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e % n);
    if (i > j) {
        m0[e] = m0[(int64_t)j * n + i];
        m1[e] = m1[(int64_t)j * n + i];
    }
}

// ascending order of the encodings = ascending order of the doubles (-0 before +0)
__device__ __forceinline__ uint64_t enc(double z) {
    const uint64_t u = (uint64_t)__double_as_longlong(z);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec(uint64_t e) {
    const uint64_t u = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    return __longlong_as_double((long long)u);
}

__global__ void __launch_bounds__(BLOCK) k_pr_depth_keys(const int64_t *__restrict__ off, int n_images,
                                                         const int *__restrict__ obs_point, int n_obs,
                                                         const double *__restrict__ rot,
                                                         const double *__restrict__ trans,
                                                         const double *__restrict__ xyz, uint64_t *keys) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_obs) return;
    const int i = image_of(off, n_images, j);
    const double *R = rot + 9 * (size_t)i;
    const double *p = xyz + 3 * (size_t)obs_point[j];
    keys[j] = enc(((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]) + trans[3 * (size_t)i + 2]);
}

__global__ void __launch_bounds__(BLOCK) k_pr_pick(const int64_t *__restrict__ off, int n_images,
                                                   const uint64_t *__restrict__ sorted, int nf,
                                                   const double *__restrict__ frac, double *z_at) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n_images * nf) return;
    const int i = e / nf, k = e % nf;
    const int64_t n = off[i + 1] - off[i];
    double z = 0.0;
    if (n > 0) {
        int64_t idx = (int64_t)((double)n * frac[k]);
        if (idx > n - 1) idx = n - 1;
        if (idx < 0) idx = 0;
        z = dec(sorted[off[i] + idx]);
    }
    z_at[e] = z;
}

// A workgroup is 4 rows of 64 pixels: a wave stores one run of 192 bytes, and the sources of a
// workgroup's pixels lie close together in the source image.
constexpr int UD_TILE_W = 64, UD_TILE_H = 4;

template <int M>
__global__ void __launch_bounds__(UD_TILE_W *UD_TILE_H) k_pr_undistort(const apd_ud::Warp W) {
    const int x = blockIdx.x * UD_TILE_W + threadIdx.x;
    const int y = blockIdx.y * UD_TILE_H + threadIdx.y;
    if (x >= W.ow || y >= W.oh) return;
    apd_ud::warp_pixel<M>(W, x, y);
}

template <int M>
void launch_undistort(const apd_ud::Warp &W, hipStream_t s) {
    const dim3 grid((unsigned)((W.ow + UD_TILE_W - 1) / UD_TILE_W), (unsigned)((W.oh + UD_TILE_H - 1) / UD_TILE_H));
    hipLaunchKernelGGL(k_pr_undistort<M>, grid, dim3(UD_TILE_W, UD_TILE_H), 0, s, W);
}

inline int grid_for(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }

}  // namespace

struct apd_prep_ctx : DevCtx {
    apd_prep_ctx() : DevCtx("apd_prep") {}
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    // model
    DevBuf rot, trans, centres, xyz, obs_off, obs_point;
    // tracks
    DevBuf keys, keys_s, head_u, head_p, pos_u, pos_p, u_image, t_start, t_point, rec, rec_off, counts;
    // pair counts and depth ranks
    DevBuf m_shared, m_narrow, z_keys, z_sorted, frac, z_at;
    DevBuf tmp;
    // undistortion: the source and the warped image
    DevBuf ud_src, ud_dst;
    double ud_upload_ms = 0.0, ud_kernel_ms = 0.0, ud_download_ms = 0.0;
    bool has_model = false;
    int n_images = 0, n_points = 0, n_obs = 0, n_tracks = 0;
    uint64_t total = 0;
    double tracks_ms = 0.0, pairs_ms = 0.0, records_ms = 0.0, ranks_ms = 0.0;
};

static int fail(apd_prep_ctx *ctx, const std::string &msg) {
    ctx->err = msg;
    return APD_EINVAL;
}

static bool all_finite(const double *p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

template <class T>
static int scan_u(apd_prep_ctx *ctx, const T *in, T *out, size_t n) {
    size_t tb = 0;
    HIP_OK(ctx, rocprim::exclusive_scan(nullptr, tb, in, out, T(0), n, rocprim::plus<T>(), ctx->stream));
    int st = grow(ctx, ctx->tmp, tb);
    if (st) return st;
    HIP_OK(ctx, rocprim::exclusive_scan(ctx->tmp.p, tb, in, out, T(0), n, rocprim::plus<T>(), ctx->stream));
    return APD_OK;
}

extern "C" {

apd_prep_ctx *apd_prep_create(int32_t device) {
    auto *ctx = open_ctx<apd_prep_ctx>(device);
    if (!ctx) return nullptr;
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreate(&ctx->ev2) != hipSuccess || hipEventCreate(&ctx->ev3) != hipSuccess) {
        apd_prep_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void apd_prep_destroy(apd_prep_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev3) (void)hipEventDestroy(ctx->ev3);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // the buffers with it
}

const char *apd_prep_last_error(const apd_prep_ctx *ctx) {
    return ctx ? ctx->err.c_str() : "apd_prep_create failed (no such HIP device)";
}

int32_t apd_prep_set_model(apd_prep_ctx *ctx, int32_t n_images, const double *rot, const double *trans,
                           const double *centres, int64_t n_points, const double *xyz, int64_t n_obs,
                           const int64_t *obs_offset, const int32_t *obs_point) {
    if (!ctx) return APD_EINVAL;
    const char *W = "apd_prep_set_model: ";
    if (n_images < 1 || n_images > APD_PREP_MAX_IMAGES)
        return fail(ctx, std::string(W) + "n_images outside 1.." + std::to_string(APD_PREP_MAX_IMAGES));
    if (n_points < 0 || n_points > (int64_t)INT32_MAX) return fail(ctx, std::string(W) + "n_points out of range");
    if (n_obs < 0 || n_obs > (int64_t)INT32_MAX) return fail(ctx, std::string(W) + "n_obs out of range");
    if (!rot || !trans || !centres || !obs_offset) return fail(ctx, std::string(W) + "a NULL camera or offset array");
    if ((n_points > 0 && !xyz) || (n_obs > 0 && !obs_point))
        return fail(ctx, std::string(W) + "a NULL array with a non-zero count");
    if (obs_offset[0] != 0 || obs_offset[n_images] != n_obs)
        return fail(ctx, std::string(W) + "obs_offset does not run from 0 to n_obs");
    for (int i = 0; i < n_images; ++i)
        if (obs_offset[i + 1] < obs_offset[i]) return fail(ctx, std::string(W) + "obs_offset does not ascend");
    for (int64_t j = 0; j < n_obs; ++j)
        if (obs_point[j] < 0 || (int64_t)obs_point[j] >= n_points)
            return fail(ctx, std::string(W) + "observation " + std::to_string(j) + " names a point outside 0..n_points-1");
    if (!all_finite(rot, 9 * (size_t)n_images) || !all_finite(trans, 3 * (size_t)n_images) ||
        !all_finite(centres, 3 * (size_t)n_images) || !all_finite(xyz, 3 * (size_t)n_points))
        return fail(ctx, std::string(W) + "a non-finite value");

    HIP_OK(ctx, hipSetDevice(ctx->device));
    ctx->has_model = false;
    ctx->tracks_ms = 0.0;
    const int n = (int)n_obs;
    const size_t cap = (size_t)n + 1;
    int st;
    if ((st = grow(ctx, ctx->rot, 72 * (size_t)n_images)) || (st = grow(ctx, ctx->trans, 24 * (size_t)n_images)) ||
        (st = grow(ctx, ctx->centres, 24 * (size_t)n_images)) || (st = grow(ctx, ctx->xyz, 24 * (size_t)n_points)) ||
        (st = grow(ctx, ctx->obs_off, 8 * ((size_t)n_images + 1))) || (st = grow(ctx, ctx->obs_point, 4 * (size_t)n)) ||
        (st = grow(ctx, ctx->keys, 8 * cap)) || (st = grow(ctx, ctx->keys_s, 8 * cap)) ||
        (st = grow(ctx, ctx->head_u, 4 * cap)) || (st = grow(ctx, ctx->head_p, 4 * cap)) ||
        (st = grow(ctx, ctx->pos_u, 4 * cap)) || (st = grow(ctx, ctx->pos_p, 4 * cap)) ||
        (st = grow(ctx, ctx->u_image, 4 * cap)) || (st = grow(ctx, ctx->t_start, 4 * cap)) ||
        (st = grow(ctx, ctx->t_point, 4 * cap)) || (st = grow(ctx, ctx->rec, 8 * cap)) ||
        (st = grow(ctx, ctx->rec_off, 8 * cap)) || (st = grow(ctx, ctx->counts, 16)))
        return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->rot.p, rot, 72 * (size_t)n_images, hipMemcpyHostToDevice, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->trans.p, trans, 24 * (size_t)n_images, hipMemcpyHostToDevice, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->centres.p, centres, 24 * (size_t)n_images, hipMemcpyHostToDevice, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->obs_off.p, obs_offset, 8 * ((size_t)n_images + 1), hipMemcpyHostToDevice, s));
    if (n_points) HIP_OK(ctx, hipMemcpyAsync(ctx->xyz.p, xyz, 24 * (size_t)n_points, hipMemcpyHostToDevice, s));
    if (n) HIP_OK(ctx, hipMemcpyAsync(ctx->obs_point.p, obs_point, 4 * (size_t)n, hipMemcpyHostToDevice, s));
    ctx->n_images = n_images;
    ctx->n_points = (int)n_points;
    ctx->n_obs = n;
    ctx->n_tracks = 0;
    ctx->total = 0;
    if (n > 0) {
        HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
        hipLaunchKernelGGL(k_pr_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const int64_t *)ctx->obs_off.p, n_images,
                           (const int *)ctx->obs_point.p, n, (uint64_t *)ctx->keys.p);
        HIP_OK(ctx, hipGetLastError());
        unsigned end_bit = 33;  // image bits (32, the low word) + the bits of the largest point index
        while (end_bit < 64 && ((uint64_t)n_points >> (end_bit - 32)) != 0) ++end_bit;
        size_t tb = 0;
        HIP_OK(ctx, rocprim::radix_sort_keys(nullptr, tb, (uint64_t *)ctx->keys.p, (uint64_t *)ctx->keys_s.p, (size_t)n,
                                            0, end_bit, s));
        if ((st = grow(ctx, ctx->tmp, tb))) return st;
        HIP_OK(ctx, rocprim::radix_sort_keys(ctx->tmp.p, tb, (uint64_t *)ctx->keys.p, (uint64_t *)ctx->keys_s.p,
                                            (size_t)n, 0, end_bit, s));
        hipLaunchKernelGGL(k_pr_heads, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t *)ctx->keys_s.p, n,
                           (uint32_t *)ctx->head_u.p, (uint32_t *)ctx->head_p.p);
        HIP_OK(ctx, hipGetLastError());
        if ((st = scan_u<uint32_t>(ctx, (const uint32_t *)ctx->head_u.p, (uint32_t *)ctx->pos_u.p, (size_t)n)) ||
            (st = scan_u<uint32_t>(ctx, (const uint32_t *)ctx->head_p.p, (uint32_t *)ctx->pos_p.p, (size_t)n)))
            return st;
        hipLaunchKernelGGL(k_pr_tracks, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t *)ctx->keys_s.p, n,
                           (const uint32_t *)ctx->head_u.p, (const uint32_t *)ctx->head_p.p,
                           (const uint32_t *)ctx->pos_u.p, (const uint32_t *)ctx->pos_p.p, (uint32_t *)ctx->u_image.p,
                           (uint32_t *)ctx->t_start.p, (uint32_t *)ctx->t_point.p, (uint32_t *)ctx->counts.p);
        HIP_OK(ctx, hipGetLastError());
        uint32_t counts[2] = {0, 0};
        HIP_OK(ctx, hipMemcpyAsync(counts, ctx->counts.p, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        const int T = (int)counts[1];
        if (T < 1 || T > n || counts[0] < (uint32_t)T || counts[0] > (uint32_t)n) {
            ctx->err = std::string(W) + "inconsistent track counts";
            return APD_EDEVICE;
        }
        hipLaunchKernelGGL(k_pr_track_records, dim3(grid_for((int64_t)T + 1)), dim3(BLOCK), 0, s,
                           (const uint32_t *)ctx->t_start.p, T, (uint64_t *)ctx->rec.p);
        HIP_OK(ctx, hipGetLastError());
        if ((st = scan_u<uint64_t>(ctx, (const uint64_t *)ctx->rec.p, (uint64_t *)ctx->rec_off.p, (size_t)T + 1)))
            return st;
        uint64_t total = 0;
        HIP_OK(ctx, hipMemcpyAsync(&total, (uint64_t *)ctx->rec_off.p + T, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ctx->tracks_ms))) return st;
        ctx->n_tracks = T;
        ctx->total = total;
    } else {
        HIP_OK(ctx, hipStreamSynchronize(s));
    }
    ctx->has_model = true;
    return APD_OK;
}

int32_t apd_prep_pair_counts(apd_prep_ctx *ctx, double q_gate, int32_t atomics, uint32_t *shared, uint32_t *narrow,
                             uint64_t *n_records) {
    if (!ctx) return APD_EINVAL;
    if (!ctx->has_model) {
        ctx->err = "apd_prep_pair_counts: no apd_prep_set_model before";
        return APD_ESTATE;
    }
    if (!shared) return fail(ctx, "apd_prep_pair_counts: NULL shared");
    if (q_gate != q_gate) return fail(ctx, "apd_prep_pair_counts: q_gate is NaN");
    if (atomics < APD_PREP_ATOMICS_DEFAULT || atomics > APD_PREP_ATOMICS_LDS)
        return fail(ctx, "apd_prep_pair_counts: unknown atomics mode");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = ctx->n_images;
    const size_t mbytes = 4 * (size_t)n * (size_t)n;
    int st;
    if ((st = grow(ctx, ctx->m_shared, mbytes)) || (st = grow(ctx, ctx->m_narrow, mbytes))) return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    HIP_OK(ctx, hipMemsetAsync(ctx->m_shared.p, 0, mbytes, s));
    HIP_OK(ctx, hipMemsetAsync(ctx->m_narrow.p, 0, mbytes, s));
    if (ctx->total > 0) {
        PairArgs A;
        A.rec_off = (const uint64_t *)ctx->rec_off.p;
        A.t_start = (const uint32_t *)ctx->t_start.p;
        A.t_point = (const uint32_t *)ctx->t_point.p;
        A.u_image = (const uint32_t *)ctx->u_image.p;
        A.centres = (const double *)ctx->centres.p;
        A.xyz = (const double *)ctx->xyz.p;
        A.shared = (uint32_t *)ctx->m_shared.p;
        A.narrow = (uint32_t *)ctx->m_narrow.p;
        A.total = ctx->total;
        A.q_gate = q_gate;
        A.n_tracks = ctx->n_tracks;
        A.n_images = n;
        const uint64_t tiles = (ctx->total + TILE - 1) / TILE;
        const int grid = (int)std::min<uint64_t>(tiles, PAIR_GRID);
        HIP_OK(ctx, hipEventRecord(ctx->ev2, s));
        // Default: aggregate in LDS when the image pairs are hot on average. A tile of TILE records
        // then holds few distinct pairs and one global atomic stands for many records (2.4x at 40
        // images with 2 000 records per pair); with many images or very long tracks nearly every
        // record of a tile has a pair of its own and the table only costs (0.5x), DESIGN section 13.
        if (atomics == APD_PREP_ATOMICS_DEFAULT) {
            const double pairs = 0.5 * (double)n * (double)(n - 1);
            atomics = (double)ctx->total >= 32.0 * pairs ? APD_PREP_ATOMICS_LDS : APD_PREP_ATOMICS_GLOBAL;
        }
        if (atomics == APD_PREP_ATOMICS_GLOBAL)
            hipLaunchKernelGGL(k_pr_pairs<false>, dim3(grid), dim3(BLOCK), 0, s, A);
        else
            hipLaunchKernelGGL(k_pr_pairs<true>, dim3(grid), dim3(BLOCK), 0, s, A);
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipEventRecord(ctx->ev3, s));
        hipLaunchKernelGGL(k_pr_mirror, dim3(grid_for((int64_t)n * n)), dim3(BLOCK), 0, s, (uint32_t *)ctx->m_shared.p,
                           (uint32_t *)ctx->m_narrow.p, n);
        HIP_OK(ctx, hipGetLastError());
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(shared, ctx->m_shared.p, mbytes, hipMemcpyDefault, s));
    if (narrow) HIP_OK(ctx, hipMemcpyAsync(narrow, ctx->m_narrow.p, mbytes, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ctx->pairs_ms))) return st;
    ctx->records_ms = 0.0;
    if (ctx->total > 0 && (st = event_ms(ctx, ctx->ev2, ctx->ev3, ctx->records_ms))) return st;
    if (n_records) *n_records = ctx->total;
    return APD_OK;
}

int32_t apd_prep_depth_ranks(apd_prep_ctx *ctx, int32_t num_fractions, const double *fractions, double *z_at,
                             int64_t *n_obs_out) {
    if (!ctx) return APD_EINVAL;
    if (!ctx->has_model) {
        ctx->err = "apd_prep_depth_ranks: no apd_prep_set_model before";
        return APD_ESTATE;
    }
    if (num_fractions < 1 || num_fractions > 64) return fail(ctx, "apd_prep_depth_ranks: num_fractions outside 1..64");
    if (!fractions || !z_at) return fail(ctx, "apd_prep_depth_ranks: NULL fractions or z_at");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    double hf[64];
    HIP_OK(ctx, hipMemcpyAsync(hf, fractions, 8 * (size_t)num_fractions, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    for (int k = 0; k < num_fractions; ++k)
        if (!(hf[k] >= 0.0 && hf[k] < 1.0)) return fail(ctx, "apd_prep_depth_ranks: a fraction outside [0, 1)");
    const int n = ctx->n_obs, ni = ctx->n_images;
    const size_t cap = (size_t)n + 1, out_n = (size_t)ni * (size_t)num_fractions;
    int st;
    if ((st = grow(ctx, ctx->z_keys, 8 * cap)) || (st = grow(ctx, ctx->z_sorted, 8 * cap)) ||
        (st = grow(ctx, ctx->frac, 8 * 64)) || (st = grow(ctx, ctx->z_at, 8 * out_n)))
        return st;
    HIP_OK(ctx, hipMemcpyAsync(ctx->frac.p, hf, 8 * (size_t)num_fractions, hipMemcpyHostToDevice, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    const int64_t *off = (const int64_t *)ctx->obs_off.p;
    if (n > 0) {
        hipLaunchKernelGGL(k_pr_depth_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, off, ni, (const int *)ctx->obs_point.p,
                           n, (const double *)ctx->rot.p, (const double *)ctx->trans.p, (const double *)ctx->xyz.p,
                           (uint64_t *)ctx->z_keys.p);
        HIP_OK(ctx, hipGetLastError());
        size_t tb = 0;
        HIP_OK(ctx, rocprim::segmented_radix_sort_keys(nullptr, tb, (uint64_t *)ctx->z_keys.p, (uint64_t *)ctx->z_sorted.p,
                                                      (unsigned)n, (unsigned)ni, off, off + 1, 0, 64, s));
        if ((st = grow(ctx, ctx->tmp, tb))) return st;
        HIP_OK(ctx, rocprim::segmented_radix_sort_keys(ctx->tmp.p, tb, (uint64_t *)ctx->z_keys.p,
                                                      (uint64_t *)ctx->z_sorted.p, (unsigned)n, (unsigned)ni, off,
                                                      off + 1, 0, 64, s));
    }
    hipLaunchKernelGGL(k_pr_pick, dim3(grid_for((int64_t)out_n)), dim3(BLOCK), 0, s, off, ni,
                       (const uint64_t *)ctx->z_sorted.p, (int)num_fractions, (const double *)ctx->frac.p,
                       (double *)ctx->z_at.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(z_at, ctx->z_at.p, 8 * out_n, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ctx->ranks_ms))) return st;
    if (n_obs_out) {
        std::vector<int64_t> ho((size_t)ni + 1);
        HIP_OK(ctx, hipMemcpy(ho.data(), ctx->obs_off.p, 8 * ((size_t)ni + 1), hipMemcpyDeviceToHost));
        for (int i = 0; i < ni; ++i) n_obs_out[i] = ho[i + 1] - ho[i];
    }
    return APD_OK;
}

int32_t apd_prep_get_timing(apd_prep_ctx *ctx, double *tracks_ms, double *pairs_ms, double *records_ms,
                            double *ranks_ms) {
    if (!ctx) return APD_EINVAL;
    if (tracks_ms) *tracks_ms = ctx->tracks_ms;
    if (pairs_ms) *pairs_ms = ctx->pairs_ms;
    if (records_ms) *records_ms = ctx->records_ms;
    if (ranks_ms) *ranks_ms = ctx->ranks_ms;
    return APD_OK;
}

int32_t apd_prep_undistort_bgr8(apd_prep_ctx *ctx, int32_t model_id, const double *params, int32_t n_params,
                                int32_t src_w, int32_t src_h, const uint8_t *src, const double *out_K, int32_t out_w,
                                int32_t out_h, uint8_t *dst) {
    if (!ctx) return APD_EINVAL;
    if (const char *what = apd_ud::check_warp(model_id, params, n_params, src_w, src_h, src, out_K, out_w, out_h, dst))
        return fail(ctx, std::string("apd_prep_undistort_bgr8: ") + what);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const size_t src_bytes = 3 * (size_t)src_w * (size_t)src_h, dst_bytes = 3 * (size_t)out_w * (size_t)out_h;
    int st;
    if ((st = grow(ctx, ctx->ud_src, src_bytes)) || (st = grow(ctx, ctx->ud_dst, dst_bytes))) return st;
    apd_ud::Warp W;
    apd_ud::fill_warp(W, params, n_params, src_w, src_h, (const uint8_t *)ctx->ud_src.p, out_K, out_w, out_h,
                      (uint8_t *)ctx->ud_dst.p);
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->ud_src.p, src, src_bytes, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev2, s));
    switch (model_id) {
        case apd_ud::SIMPLE_PINHOLE: launch_undistort<apd_ud::SIMPLE_PINHOLE>(W, s); break;
        case apd_ud::PINHOLE: launch_undistort<apd_ud::PINHOLE>(W, s); break;
        case apd_ud::SIMPLE_RADIAL: launch_undistort<apd_ud::SIMPLE_RADIAL>(W, s); break;
        case apd_ud::RADIAL: launch_undistort<apd_ud::RADIAL>(W, s); break;
        case apd_ud::OPENCV: launch_undistort<apd_ud::OPENCV>(W, s); break;
        case apd_ud::OPENCV_FISHEYE: launch_undistort<apd_ud::OPENCV_FISHEYE>(W, s); break;
        case apd_ud::FULL_OPENCV: launch_undistort<apd_ud::FULL_OPENCV>(W, s); break;
        case apd_ud::SIMPLE_RADIAL_FISHEYE: launch_undistort<apd_ud::SIMPLE_RADIAL_FISHEYE>(W, s); break;
        case apd_ud::RADIAL_FISHEYE: launch_undistort<apd_ud::RADIAL_FISHEYE>(W, s); break;
        default: launch_undistort<apd_ud::THIN_PRISM_FISHEYE>(W, s); break;
    }
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev3, s));
    HIP_OK(ctx, hipMemcpyAsync(dst, ctx->ud_dst.p, dst_bytes, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = event_ms(ctx, ctx->ev0, ctx->ev2, ctx->ud_upload_ms)) ||
        (st = event_ms(ctx, ctx->ev2, ctx->ev3, ctx->ud_kernel_ms)))
        return st;
    return event_ms(ctx, ctx->ev3, ctx->ev1, ctx->ud_download_ms);
}

int32_t apd_prep_get_undistort_timing(apd_prep_ctx *ctx, double *upload_ms, double *kernel_ms, double *download_ms) {
    if (!ctx) return APD_EINVAL;
    if (upload_ms) *upload_ms = ctx->ud_upload_ms;
    if (kernel_ms) *kernel_ms = ctx->ud_kernel_ms;
    if (download_ms) *download_ms = ctx->ud_download_ms;
    return APD_OK;
}

double apd_prep_cos_gate(double degrees) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!(degrees > 0.0 && degrees <= 180.0)) return nan;
    const double k = 180.0 / 3.14159265358979323846;
    auto lt = [&](double q) { return k * acos(q) < degrees; };
    auto bits = [](double d) {
        int64_t b;
        memcpy(&b, &d, 8);
        return b < 0 ? (int64_t)(0x8000000000000000ull - (uint64_t)b) : b;  // monotone in d
    };
    auto from = [](int64_t m) {
        const int64_t b = m < 0 ? (int64_t)(0x8000000000000000ull - (uint64_t)m) : m;
        double d;
        memcpy(&d, &b, 8);
        return d;
    };
    if (lt(-1.0)) return -1.0;  // degrees > 180 rounded: every q in [-1, 1] passes
    if (!lt(1.0)) return nan;
    int64_t lo = bits(-1.0), hi = bits(1.0);  // lt(lo) false, lt(hi) true
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (lt(from(mid))) hi = mid; else lo = mid;
    }
    for (int i = 1; i <= 64; ++i) {
        if (hi + i <= bits(1.0) && !lt(from(hi + i))) return nan;
        if (lo - i >= bits(-1.0) && lt(from(lo - i))) return nan;
    }
    return from(hi);
}

}  // extern "C"
