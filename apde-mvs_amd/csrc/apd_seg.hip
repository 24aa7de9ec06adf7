// apd_seg.hip — the device side of include/apd_seg.h: flat-zone sa_masks by connected components.
//
// k_seg_downscale      one working pixel per lane: the rounded box mean (only when s > 1)
// k_seg_smooth_flat    a 64 x 16 tile of the working image with a halo of 3 in LDS (2 for the filter, 1
//                      for the neighbour test): T, S and the flat byte; the S planes reach memory only
//                      for apd_seg_get_stage
// k_seg_ccl_tile       union-find over one tile, parents in LDS; each flat pixel then holds the global
//                      index of its tile-local root (the tile component's smallest index), others -1
// k_seg_ccl_merge      one lane per pair of 4-neighbours on either side of a tile border: find / atomicMin
//                      on the global parents, the larger root always hung under the smaller, so the
//                      final root is the component's smallest index whatever the order of the atomics
// k_seg_flatten_area   per tile: pixels counted per tile-local component in LDS, then one chain walk and
//                      one global integer atomic per tile-local component; roots written per pixel
// ranking              rocprim inclusive scan of (area >= min_area) -> k_seg_compact writes the survivors'
//                      keys in root order -> rocprim radix sort -> the first 255 keys go to the host,
//                      which builds the root -> label table (apd_sg::table_from_ranked)
// k_seg_relabel        table in LDS, a binary search per flat pixel
//
// Integer atomics only (min and add), so every output is the same from run to run.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/apd_seg.h"
#include "apd_host.h"
#include "apd_seg.h"

namespace {

using namespace apd_sg;

constexpr int TW = 64, TH = 16;            // the tile of every tiled kernel
constexpr int BLOCK = 256;                 // its workgroup: 4 pixels per lane
constexpr int PER_LANE = TW * TH / BLOCK;  // lane t has the pixels t + BLOCK*k: column t % 64, rows t/64 + 4k

__global__ void __launch_bounds__(BLOCK) k_seg_downscale(const uint8_t *src, int w, int h, int s, uint8_t *work, int W,
                                                         int H) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const int X = (int)(i % W), Y = (int)(i / W);
    for (int c = 0; c < 3; ++c) work[i * 3 + c] = box_mean(src, w, h, s, X, Y, c);
}

constexpr int IN_W = TW + 6, IN_H = TH + 6;  // the working image with a halo of 3
constexpr int S_W = TW + 2, S_H = TH + 2;    // S with a halo of 1

template <bool WRITE_S>
__global__ void __launch_bounds__(BLOCK) k_seg_smooth_flat(const uint8_t *work, int W, int H, int threshold_q8,
                                                           uint8_t *flat, uint16_t *smooth) {
    __shared__ uint8_t in[IN_H][IN_W][3];
    __shared__ uint16_t hor[3][IN_H][S_W];  // T: column j is pixel tx0 - 1 + j, row i is pixel row clamp(ty0 - 3 + i)
    __shared__ uint16_t sm[3][S_H][S_W];    // S: column j is pixel tx0 - 1 + j, row i is pixel row ty0 - 1 + i
    const int tid = threadIdx.x, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    for (int i = tid; i < IN_H * IN_W; i += BLOCK) {
        const int r = i / IN_W, c = i % IN_W;
        const int gy = clampi(ty0 - 3 + r, 0, H - 1), gx = clampi(tx0 - 3 + c, 0, W - 1);
        const uint8_t *p = work + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
        in[r][c][0] = p[0];
        in[r][c][1] = p[1];
        in[r][c][2] = p[2];
    }
    __syncthreads();
    for (int i = tid; i < IN_H * S_W; i += BLOCK) {
        const int r = i / S_W, c = i % S_W;
        for (int ch = 0; ch < 3; ++ch)
            hor[ch][r][c] = (uint16_t)tap5(in[r][c][ch], in[r][c + 1][ch], in[r][c + 2][ch], in[r][c + 3][ch], in[r][c + 4][ch]);
    }
    __syncthreads();
    for (int i = tid; i < S_H * S_W; i += BLOCK) {
        const int r = i / S_W, c = i % S_W;
        for (int ch = 0; ch < 3; ++ch)
            sm[ch][r][c] = (uint16_t)tap5(hor[ch][r][c], hor[ch][r + 1][c], hor[ch][r + 2][c], hor[ch][r + 3][c], hor[ch][r + 4][c]);
    }
    __syncthreads();
    const size_t N = (size_t)W * (size_t)H;
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, lx = l % TW, ly = l / TW;
        const int gx = tx0 + lx, gy = ty0 + ly;
        if (gx >= W || gy >= H) continue;
        const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
        if (WRITE_S) {
            for (int ch = 0; ch < 3; ++ch) smooth[(size_t)ch * N + g] = sm[ch][ly + 1][lx + 1];
            continue;
        }
        int worst = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = gx + dx, qy = gy + dy;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                for (int ch = 0; ch < 3; ++ch) {
                    const int d = absdiff(sm[ch][ly + 1][lx + 1], sm[ch][ly + 1 + dy][lx + 1 + dx]);
                    worst = d > worst ? d : worst;
                }
            }
        flat[g] = worst <= threshold_q8 ? 1 : 0;
    }
}

// Union-find on parents with parent[i] <= i, safe against concurrent unions: a stale read is an
// earlier ancestor of the same tree, and the atomicMin on what was believed a root tells if it was.
template <bool GLOBAL>
__device__ __forceinline__ int uf_load(int *p, int i) {
    return GLOBAL ? __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int uf_find(int *p, int a) {
    for (int up = uf_load<GLOBAL>(p, a); up != a; up = uf_load<GLOBAL>(p, a)) a = up;
    return a;
}
template <bool GLOBAL>
__device__ __forceinline__ void uf_unite(int *p, int a, int b) {
    for (;;) {
        a = uf_find<GLOBAL>(p, a);
        b = uf_find<GLOBAL>(p, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(p + b, a);  // b was a root if it still pointed at itself
        if (old == b) return;
        b = old;  // it was not: what it pointed at joins a's tree instead
    }
}

__global__ void __launch_bounds__(BLOCK) k_seg_ccl_tile(const uint8_t *flat, int W, int H, int *parent) {
    __shared__ int par[TW * TH];
    const int tid = threadIdx.x, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, gx = tx0 + l % TW, gy = ty0 + l / TW;
        const bool on = gx < W && gy < H && flat[(size_t)gy * (size_t)W + (size_t)gx] != 0;
        par[l] = on ? l : -1;
    }
    __syncthreads();
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, lx = l % TW, ly = l / TW;
        if (par[l] < 0) continue;  // the sign of a parent never changes
        if (lx > 0 && par[l - 1] >= 0) uf_unite<false>(par, l, l - 1);
        if (ly > 0 && par[l - TW] >= 0) uf_unite<false>(par, l, l - TW);
    }
    __syncthreads();
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, gx = tx0 + l % TW, gy = ty0 + l / TW;
        if (gx >= W || gy >= H) continue;
        int out = -1;
        if (par[l] >= 0) {
            int r = l;
            while (par[r] != r) r = par[r];
            out = (ty0 + r / TW) * W + tx0 + r % TW;  // local and global order agree inside a tile
        }
        parent[(size_t)gy * (size_t)W + (size_t)gx] = out;
    }
}

__global__ void __launch_bounds__(BLOCK) k_seg_ccl_merge(int *parent, int W, int H, int64_t n_vertical, int64_t n_pairs) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_pairs) return;
    int64_t a, q;
    if (i < n_vertical) {  // the pixel right of a vertical border and its left neighbour
        const int64_t x = (i / H + 1) * TW, y = i % H;
        a = y * W + x;
        q = a - 1;
    } else {  // the pixel below a horizontal border and its upper neighbour
        const int64_t j = i - n_vertical, y = (j / W + 1) * TH, x = j % W;
        a = y * W + x;
        q = a - W;
    }
    if (parent[a] >= 0 && parent[q] >= 0) uf_unite<true>(parent, (int)a, (int)q);
}

__global__ void __launch_bounds__(BLOCK) k_seg_flatten_area(const int *parent, int W, int H, int *roots, int *area) {
    __shared__ int cnt[TW * TH];
    __shared__ int root_of[TW * TH];
    const int tid = threadIdx.x, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    for (int k = 0; k < PER_LANE; ++k) cnt[tid + BLOCK * k] = 0;
    __syncthreads();
    int key[PER_LANE];
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, gx = tx0 + l % TW, gy = ty0 + l / TW;
        key[k] = -1;
        if (gx >= W || gy >= H) continue;
        const int p = parent[(size_t)gy * (size_t)W + (size_t)gx];
        if (p < 0) continue;
        // a pixel points at its tile-local root; a tile-local root the merge has hung elsewhere counts
        // under itself (or under a pixel of its own component in this tile: the sum is the same)
        const int px = p % W - tx0, py = p / W - ty0;
        key[k] = (px >= 0 && px < TW && py >= 0 && py < TH) ? py * TW + px : l;
        atomicAdd(&cnt[key[k]], 1);
    }
    __syncthreads();
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k;
        if (cnt[l] == 0) continue;
        int r = (ty0 + l / TW) * W + tx0 + l % TW;
        for (int up = parent[r]; up != r; up = parent[r]) r = up;
        root_of[l] = r;
        atomicAdd(area + r, cnt[l]);
    }
    __syncthreads();
    for (int k = 0; k < PER_LANE; ++k) {
        const int l = tid + BLOCK * k, gx = tx0 + l % TW, gy = ty0 + l / TW;
        if (gx >= W || gy >= H) continue;
        roots[(size_t)gy * (size_t)W + (size_t)gx] = key[k] >= 0 ? root_of[key[k]] : -1;
    }
}

struct IsSurvivor {
    int min_area;
    __host__ __device__ int operator()(int a) const { return a >= min_area ? 1 : 0; }
};

__global__ void __launch_bounds__(BLOCK) k_seg_compact(const int *area, const int *rank_incl, int min_area, int64_t N,
                                                       uint64_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const int a = area[i];
    if (a >= min_area) keys[rank_incl[i] - 1] = ((uint64_t)(0xFFFFFFFFu - (uint32_t)a) << 32) | (uint32_t)i;
}

__global__ void __launch_bounds__(BLOCK) k_seg_relabel(const int *roots, int64_t N, const LabelTable table, uint8_t *labels) {
    __shared__ int32_t t_root[APD_SEG_MAX_LABELS];
    __shared__ uint8_t t_label[APD_SEG_MAX_LABELS];
    if ((int)threadIdx.x < table.n) {
        t_root[threadIdx.x] = table.root[threadIdx.x];
        t_label[threadIdx.x] = table.label[threadIdx.x];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const int r = roots[i];
    labels[i] = r >= 0 ? label_of(t_root, t_label, table.n, r) : (uint8_t)0;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

constexpr int NUM_EVENTS = APD_SEG_NUM_TIMES + 1;

}  // namespace

struct apd_seg_ctx : DevCtx {
    apd_seg_ctx() : DevCtx("apd_seg") {}
    hipEvent_t ev[NUM_EVENTS] = {};
    DevBuf src, work, smooth, flat, parent, roots, area, keys, keys_sorted, labels, tmp;
    int last = 0;  // 0: no call yet, 1: apd_seg_label_mask, 2: apd_seg_flat_zones_bgr8
    int W = 0, H = 0;
    double ms[APD_SEG_NUM_TIMES] = {};
};

static int fail(apd_seg_ctx *ctx, const std::string &msg) {
    ctx->err = msg;
    return APD_EINVAL;
}

// Stage 4 and the areas on ctx->flat: events 3 (on entry) to 6. Leaves roots and area.
static int run_components(apd_seg_ctx *ctx, int W, int H) {
    hipStream_t s = ctx->stream;
    const size_t N = (size_t)W * (size_t)H;
    int st;
    if ((st = grow(ctx, ctx->parent, N * 4)) || (st = grow(ctx, ctx->roots, N * 4)) || (st = grow(ctx, ctx->area, N * 4)))
        return st;
    const int ntx = ceil_div(W, TW), nty = ceil_div(H, TH);
    const dim3 tiles((unsigned)ntx, (unsigned)nty);
    HIP_OK(ctx, hipEventRecord(ctx->ev[3], s));
    hipLaunchKernelGGL(k_seg_ccl_tile, tiles, dim3(BLOCK), 0, s, (const uint8_t *)ctx->flat.p, W, H, (int *)ctx->parent.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev[4], s));
    const int64_t n_vertical = (int64_t)(ntx - 1) * H, n_pairs = n_vertical + (int64_t)(nty - 1) * W;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_seg_ccl_merge, dim3(blocks_for(n_pairs)), dim3(BLOCK), 0, s, (int *)ctx->parent.p, W, H,
                           n_vertical, n_pairs);
        HIP_OK(ctx, hipGetLastError());
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev[5], s));
    HIP_OK(ctx, hipMemsetAsync(ctx->area.p, 0, N * 4, s));
    hipLaunchKernelGGL(k_seg_flatten_area, tiles, dim3(BLOCK), 0, s, (const int *)ctx->parent.p, W, H, (int *)ctx->roots.p,
                       (int *)ctx->area.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev[6], s));
    return APD_OK;
}

static int read_times(apd_seg_ctx *ctx) {
    int st = APD_OK;
    for (int k = 0; !st && k < APD_SEG_NUM_TIMES; ++k) st = event_ms(ctx, ctx->ev[k], ctx->ev[k + 1], ctx->ms[k]);
    return st;
}

extern "C" {

apd_seg_ctx *apd_seg_create(int32_t device) {
    auto *ctx = open_ctx<apd_seg_ctx>(device);
    if (!ctx) return nullptr;
    bool ok = true;
    for (int k = 0; ok && k < NUM_EVENTS; ++k) ok = hipEventCreate(&ctx->ev[k]) == hipSuccess;
    if (!ok) {
        apd_seg_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void apd_seg_destroy(apd_seg_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipEvent_t e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // the buffers with it
}

const char *apd_seg_last_error(const apd_seg_ctx *ctx) {
    return ctx ? ctx->err.c_str() : "apd_seg_create failed (no such HIP device)";
}

int32_t apd_seg_label_mask(apd_seg_ctx *ctx, int32_t W, int32_t H, const uint8_t *mask_u8, int32_t *roots_i32) {
    if (!ctx) return APD_EINVAL;
    if (const char *what = check_label_mask(W, H, mask_u8, roots_i32))
        return fail(ctx, std::string("apd_seg_label_mask: ") + what);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    ctx->last = 0;
    const size_t N = (size_t)W * (size_t)H;
    int st;
    if ((st = grow(ctx, ctx->flat, N))) return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipEventRecord(ctx->ev[0], s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->flat.p, mask_u8, N, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[1], s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[2], s));
    if ((st = run_components(ctx, W, H))) return st;
    HIP_OK(ctx, hipEventRecord(ctx->ev[7], s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[8], s));
    HIP_OK(ctx, hipMemcpyAsync(roots_i32, ctx->roots.p, N * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[9], s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = read_times(ctx))) return st;
    ctx->W = W;
    ctx->H = H;
    ctx->last = 1;
    return APD_OK;
}

int32_t apd_seg_flat_zones_bgr8(apd_seg_ctx *ctx, int32_t w, int32_t h, const uint8_t *src, int32_t max_size,
                                int32_t threshold_q8, int32_t min_area, uint8_t *labels, int32_t *out_w,
                                int32_t *out_h, int32_t *n_survivors, int32_t *n_labels) {
    if (!ctx) return APD_EINVAL;
    if (const char *what = check_flat_zones(w, h, src, max_size, threshold_q8, min_area, labels, out_w, out_h))
        return fail(ctx, std::string("apd_seg_flat_zones_bgr8: ") + what);
    HIP_OK(ctx, hipSetDevice(ctx->device));
    ctx->last = 0;
    const int f = scale_of(w, h, max_size);
    const int W = ceil_div(w, f), H = ceil_div(h, f);
    const size_t N = (size_t)W * (size_t)H, src_bytes = 3 * (size_t)w * (size_t)h;
    int st;
    if ((st = grow(ctx, ctx->work, 3 * N)) || (st = grow(ctx, ctx->flat, N)) || (st = grow(ctx, ctx->labels, N))) return st;
    if (f > 1 && (st = grow(ctx, ctx->src, src_bytes))) return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipEventRecord(ctx->ev[0], s));
    HIP_OK(ctx, hipMemcpyAsync(f > 1 ? ctx->src.p : ctx->work.p, src, src_bytes, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[1], s));
    if (f > 1) {
        hipLaunchKernelGGL(k_seg_downscale, dim3(blocks_for((int64_t)N)), dim3(BLOCK), 0, s, (const uint8_t *)ctx->src.p, w,
                           h, f, (uint8_t *)ctx->work.p, W, H);
        HIP_OK(ctx, hipGetLastError());
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev[2], s));
    const dim3 tiles((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH));
    hipLaunchKernelGGL(k_seg_smooth_flat<false>, tiles, dim3(BLOCK), 0, s, (const uint8_t *)ctx->work.p, W, H,
                       threshold_q8, (uint8_t *)ctx->flat.p, (uint16_t *)nullptr);
    HIP_OK(ctx, hipGetLastError());
    if ((st = run_components(ctx, W, H))) return st;

    // ranking: the survivors' keys in root order, sorted; the parents are dead and hold the scan
    int *rank_incl = (int *)ctx->parent.p;
    const auto flags = rocprim::make_transform_iterator((const int *)ctx->area.p, IsSurvivor{min_area});
    size_t tb = 0;
    HIP_OK(ctx, rocprim::inclusive_scan(nullptr, tb, flags, rank_incl, N, rocprim::plus<int>(), s));
    if ((st = grow(ctx, ctx->tmp, tb))) return st;
    HIP_OK(ctx, rocprim::inclusive_scan(ctx->tmp.p, tb, flags, rank_incl, N, rocprim::plus<int>(), s));
    int survivors = 0;
    HIP_OK(ctx, hipMemcpyAsync(&survivors, rank_incl + (N - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const int top = survivors < APD_SEG_MAX_LABELS ? survivors : APD_SEG_MAX_LABELS;
    uint64_t ranked[APD_SEG_MAX_LABELS];
    if (survivors > 0) {
        const size_t key_bytes = (size_t)survivors * sizeof(uint64_t);
        if ((st = grow(ctx, ctx->keys, key_bytes)) || (st = grow(ctx, ctx->keys_sorted, key_bytes))) return st;
        hipLaunchKernelGGL(k_seg_compact, dim3(blocks_for((int64_t)N)), dim3(BLOCK), 0, s, (const int *)ctx->area.p,
                           (const int *)rank_incl, min_area, (int64_t)N, (uint64_t *)ctx->keys.p);
        HIP_OK(ctx, hipGetLastError());
        tb = 0;
        HIP_OK(ctx, rocprim::radix_sort_keys(nullptr, tb, (const uint64_t *)ctx->keys.p, (uint64_t *)ctx->keys_sorted.p,
                                            (size_t)survivors, 0, 64, s));
        if ((st = grow(ctx, ctx->tmp, tb))) return st;
        HIP_OK(ctx, rocprim::radix_sort_keys(ctx->tmp.p, tb, (const uint64_t *)ctx->keys.p, (uint64_t *)ctx->keys_sorted.p,
                                            (size_t)survivors, 0, 64, s));
        HIP_OK(ctx, hipMemcpyAsync(ranked, ctx->keys_sorted.p, (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
    }
    LabelTable table;
    table_from_ranked(ranked, top, table);
    HIP_OK(ctx, hipEventRecord(ctx->ev[7], s));
    hipLaunchKernelGGL(k_seg_relabel, dim3(blocks_for((int64_t)N)), dim3(BLOCK), 0, s, (const int *)ctx->roots.p, (int64_t)N,
                       table, (uint8_t *)ctx->labels.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev[8], s));
    HIP_OK(ctx, hipMemcpyAsync(labels, ctx->labels.p, N, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev[9], s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = read_times(ctx))) return st;
    *out_w = W;
    *out_h = H;
    if (n_survivors) *n_survivors = survivors;
    if (n_labels) *n_labels = top;
    ctx->W = W;
    ctx->H = H;
    ctx->last = 2;
    return APD_OK;
}

int32_t apd_seg_get_stage(apd_seg_ctx *ctx, int32_t which, void *out) {
    if (!ctx) return APD_EINVAL;
    if (which < APD_SEG_STAGE_WORK || which > APD_SEG_STAGE_AREAS) return fail(ctx, "apd_seg_get_stage: an unknown stage");
    if (!out) return fail(ctx, "apd_seg_get_stage: a NULL pointer");
    if (ctx->last == 0 || (ctx->last == 1 && which <= APD_SEG_STAGE_SMOOTH)) {
        ctx->err = "apd_seg_get_stage: the last call left no such stage";
        return APD_ESTATE;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    const size_t N = (size_t)W * (size_t)H;
    hipStream_t s = ctx->stream;
    const void *from = nullptr;
    size_t bytes = 0;
    switch (which) {
        case APD_SEG_STAGE_WORK: from = ctx->work.p; bytes = 3 * N; break;
        case APD_SEG_STAGE_SMOOTH: {  // not kept by the call: the same kernel once more, writing S
            int st = grow(ctx, ctx->smooth, 6 * N);
            if (st) return st;
            const dim3 tiles((unsigned)ceil_div(W, TW), (unsigned)ceil_div(H, TH));
            hipLaunchKernelGGL(k_seg_smooth_flat<true>, tiles, dim3(BLOCK), 0, s, (const uint8_t *)ctx->work.p, W, H, 0,
                               (uint8_t *)nullptr, (uint16_t *)ctx->smooth.p);
            HIP_OK(ctx, hipGetLastError());
            from = ctx->smooth.p;
            bytes = 6 * N;
            break;
        }
        case APD_SEG_STAGE_FLAT: from = ctx->flat.p; bytes = N; break;
        case APD_SEG_STAGE_ROOTS: from = ctx->roots.p; bytes = 4 * N; break;
        default: from = ctx->area.p; bytes = 4 * N; break;
    }
    HIP_OK(ctx, hipMemcpyAsync(out, from, bytes, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return APD_OK;
}

int32_t apd_seg_get_timing(apd_seg_ctx *ctx, double *ms) {
    if (!ctx || !ms) return APD_EINVAL;
    for (int k = 0; k < APD_SEG_NUM_TIMES; ++k) ms[k] = ctx->ms[k];
    return APD_OK;
}

}  // extern "C"
