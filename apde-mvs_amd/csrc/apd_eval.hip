// apd_eval.hip — device side of the point-cloud evaluation (include/apd_eval.h): truncated
// nearest-neighbour distances between two clouds, voxel down-sampling, and a z-buffer renderer of a
// cloud into cameras with a per-point visibility count (integer atomics: deterministic), the
// free-space gap of points against depth maps and per-voxel good / bad scores (integer sums); a crop
// volume, the nearest neighbour with its index, and point-to-point ICP whose per-iteration sums are
// taken in a fixed tree order in fp64 (the same bits every run, and the host twins' bits); exact
// radius thinning (the greedy maximal independent set of the radius graph as the fixed point of two
// final rules over a shrinking worklist), an observability mask, a half-space and masked mean /
// median statistics, the steps of the DTU protocol.
//
// Search structure: a Morton-sorted implicit bounding-volume tree.
//   - finite targets are quantised to 21 bits per axis over their bounding box (in double) and sorted
//     by the 63-bit Morton key (rocPRIM radix sort, stable, so the order is the same every run);
//   - leaves are runs of LEAF consecutive sorted points with their exact fp32 min/max box;
//   - level l+1 holds the min/max of every FAN consecutive boxes of level l, up to a single root.
//     Children are index arithmetic: node i of level l+1 covers nodes [i*FAN, i*FAN+FAN) of level l.
//   - queries are sorted by the same key so that the lanes of a wave walk the same part of the tree;
//     each lane first evaluates the leaf at its own position in the sorted target keys, which makes
//     the bound tight before the descent from the root starts.
// Compiled with -ffp-contract=off: the distance statement is the contract, bit for bit.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_scan_by_key.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/apd_eval.h"
#include "apd_dtu.h"
#include "apd_host.h"
#include "apd_register.h"

namespace {

constexpr int LEAF = 32;        // points per leaf
constexpr int FAN = 8;          // children per internal node
constexpr int MAX_LEVELS = 12;  // 32 * 8^9 > 2^31 points: at most 10 levels are ever used
// deepest stack: popping an internal node pushes at most FAN children (net +7) once per level
constexpr int STACK = 1 + (FAN - 1) * (MAX_LEVELS - 1);
constexpr int BLOCK = 256;
constexpr uint64_t KEY_NONE = ~0ull;  // non-finite point: sorts behind every 63-bit key
constexpr int TOL_CHUNK = 8;

struct Tree {
    const float4 *pts;    // sorted finite targets, w unused
    const float4 *boxes;  // per node: lo, hi
    const uint64_t *keys; // sorted Morton keys of pts
    int nf;               // finite targets
    int levels;           // number of levels, level 0 = leaves, level levels-1 = root
    int off[MAX_LEVELS];  // first node of each level in boxes (in nodes)
    int cnt[MAX_LEVELS];
};

__device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// bounds[0..2] = min, [3..5] = max of the finite points (order-preserving uint encoding; integer
// atomics, so the result does not depend on the order of arrival)
__global__ void __launch_bounds__(BLOCK) k_bounds(const float *__restrict__ xyz, int n, uint32_t *bounds) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) continue;
        const uint32_t e[3] = {f2ord(x), f2ord(y), f2ord(z)};
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], e[a]);
            hi[a] = max(hi[a], e[a]);
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int s = 32; s > 0; s >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], s));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], s));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) {
            if (lo[a] != 0xFFFFFFFFu) atomicMin(&bounds[a], lo[a]);
            if (hi[a] != 0u) atomicMax(&bounds[3 + a], hi[a]);
        }
    }
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// Morton key of a point over the target's bounding box, quantised in double; a zero extent maps the
// axis to cell 0 and points outside the box (queries) are clamped to its faces.
__device__ __forceinline__ uint32_t quant21(float v, uint32_t lo_e, uint32_t hi_e) {
    const double lo = (double)ord2f(lo_e), ext = (double)ord2f(hi_e) - lo;
    if (!(ext > 0.0)) return 0u;
    double t = ((double)v - lo) * (2097152.0 / ext);
    t = t < 0.0 ? 0.0 : (t > 2097151.0 ? 2097151.0 : t);
    return (uint32_t)t;
}

__global__ void __launch_bounds__(BLOCK) k_morton_keys(const float *__restrict__ xyz, int n,
                                                       const uint32_t *__restrict__ bounds, uint64_t *keys, int *idx,
                                                       unsigned long long *n_finite) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    bool fin = false;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        fin = finite3(x, y, z);
        uint64_t k = KEY_NONE;
        if (fin)
            k = spread21(quant21(x, bounds[0], bounds[3])) << 2 | spread21(quant21(y, bounds[1], bounds[4])) << 1 |
                spread21(quant21(z, bounds[2], bounds[5]));
        keys[i] = k;
        idx[i] = i;
    }
    if (n_finite) {  // one integer atomic per wave
        const unsigned long long m = __ballot(fin);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_finite, (unsigned long long)__popcll(m));
    }
}

__global__ void __launch_bounds__(BLOCK) k_gather_points(const float *__restrict__ xyz, const int *__restrict__ idx,
                                                         int nf, float4 *pts) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nf) return;
    const size_t s = 3 * (size_t)idx[i];
    pts[i] = make_float4(xyz[s], xyz[s + 1], xyz[s + 2], 0.0f);
}

__global__ void __launch_bounds__(BLOCK) k_leaf_boxes(const float4 *__restrict__ pts, int nf, int nleaf,
                                                      float4 *boxes) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= nleaf) return;
    const int b = l * LEAF, e = min(b + LEAF, nf);
    float4 p = pts[b];
    float lx = p.x, ly = p.y, lz = p.z, hx = p.x, hy = p.y, hz = p.z;
    for (int j = b + 1; j < e; ++j) {
        p = pts[j];
        lx = fminf(lx, p.x); ly = fminf(ly, p.y); lz = fminf(lz, p.z);
        hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y); hz = fmaxf(hz, p.z);
    }
    boxes[2 * (size_t)l] = make_float4(lx, ly, lz, 0.0f);
    boxes[2 * (size_t)l + 1] = make_float4(hx, hy, hz, 0.0f);
}

__global__ void __launch_bounds__(BLOCK) k_upper_boxes(const float4 *__restrict__ child, int nchild, int nparent,
                                                       float4 *parent) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= nparent) return;
    const int b = p * FAN, e = min(b + FAN, nchild);
    float4 lo = child[2 * (size_t)b], hi = child[2 * (size_t)b + 1];
    for (int j = b + 1; j < e; ++j) {
        const float4 l2 = child[2 * (size_t)j], h2 = child[2 * (size_t)j + 1];
        lo.x = fminf(lo.x, l2.x); lo.y = fminf(lo.y, l2.y); lo.z = fminf(lo.z, l2.z);
        hi.x = fmaxf(hi.x, h2.x); hi.y = fmaxf(hi.y, h2.y); hi.z = fmaxf(hi.z, h2.z);
    }
    parent[2 * (size_t)p] = lo;
    parent[2 * (size_t)p + 1] = hi;
}

__device__ __forceinline__ float point_d2(float qx, float qy, float qz, const float4 t) {
    const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float box_d2(float qx, float qy, float qz, const float4 lo, const float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ void eval_leaf(const Tree &T, int leaf, float qx, float qy, float qz, float &cur,
                                          bool &found) {
    const int b = leaf * LEAF, e = min(b + LEAF, T.nf);
    for (int j = b; j < e; ++j) {
        const float d2 = point_d2(qx, qy, qz, T.pts[j]);  // one 16-byte load per point
        if (d2 <= cur) {
            cur = d2;
            found = true;
        }
    }
}

// One lane per query, queries in Morton order.
//
// Exactness of the pruning. For a box [lo, hi] and a point t inside it, per axis:
//   q < lo:  lo - q <= t - q exactly, and fp32 subtraction is monotone, so fl(lo - q) <= fl(t - q)
//            = |fl(q - t)|;   q > hi: likewise with q - hi;   otherwise g = 0 <= |dx|.
// fp32 multiplication and addition of non-negative values are monotone too, and box_d2 uses the
// same statement (gx*gx + gy*gy) + gz*gz as point_d2, so box_d2 <= the COMPUTED d2 of every point
// in the box. A node is skipped iff box_d2 > cur (strict), where cur is the smallest computed d2 so
// far: nothing that could lower (or tie) the minimum is lost, with no margin.
// The cut-off applies to sqrtf(min d2), not to d2. The initial bound `bound_d2` is the LARGEST
// float b with sqrtf(b) <= max_dist, found by the host by stepping floats (not a rounded
// max_dist*max_dist): sqrtf is monotone, so every d2 whose root passes the cut-off is <= bound_d2
// and survives the pruning, and everything above it would be cut anyway.
//
// The per-lane stack (STACK entries of node + box distance) is indexed at run time and therefore
// lives in scratch memory.
__global__ void __launch_bounds__(BLOCK) k_nearest(const Tree T, int nq, const uint64_t *__restrict__ qkeys,
                                                   const int *__restrict__ qidx, const float *__restrict__ qxyz,
                                                   float bound_d2, float max_dist, float *__restrict__ dist) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nq) return;
    const int qi = qidx[i];
    const uint64_t key = qkeys[i];
    const float inf = __uint_as_float(0x7F800000u);
    if (key == KEY_NONE || T.nf == 0) {
        dist[qi] = inf;
        return;
    }
    const float qx = qxyz[3 * (size_t)qi], qy = qxyz[3 * (size_t)qi + 1], qz = qxyz[3 * (size_t)qi + 2];
    float cur = bound_d2;
    bool found = false;

    // the leaf at the query's own position in the sorted keys
    int lo = 0, hi = T.nf;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (T.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int leaf0 = min(lo, T.nf - 1) / LEAF;
    eval_leaf(T, leaf0, qx, qy, qz, cur, found);

    uint32_t st_node[STACK];  // level << 27 | index (at most 2^26 leaves)
    float st_d2[STACK];
    int sp = 0;
    if (T.levels > 1) {
        st_node[0] = (uint32_t)(T.levels - 1) << 27;
        st_d2[0] = 0.0f;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        if (st_d2[sp] > cur) continue;
        const int lvl = (int)(st_node[sp] >> 27), idx = (int)(st_node[sp] & 0x7FFFFFFu);
        const int cl = lvl - 1;
        const int b = idx * FAN, e = min(b + FAN, T.cnt[cl]);
        const float4 *cb = T.boxes + 2 * (size_t)T.off[cl];
        for (int c = b; c < e; ++c) {
            const float bd = box_d2(qx, qy, qz, cb[2 * (size_t)c], cb[2 * (size_t)c + 1]);
            if (bd > cur) continue;
            if (cl == 0) {
                if (c != leaf0) eval_leaf(T, c, qx, qy, qz, cur, found);
            } else if (sp < STACK) {  // always true (see STACK); keeps the store in bounds regardless
                st_node[sp] = (uint32_t)cl << 27 | (uint32_t)c;
                st_d2[sp] = bd;
                ++sp;
            }
        }
    }
    float r = inf;
    if (found) {
        const float m = sqrtf(cur);
        if (m <= max_dist) r = m;
    }
    dist[qi] = r;
}

// within[k] += #{dist <= tol[k]} for up to TOL_CHUNK tolerances: per-lane integer counts over a
// grid-stride loop, a wave reduction, then one integer atomic per wave and tolerance.
struct TolChunk {
    float tol[TOL_CHUNK];
    int n;
};
__global__ void __launch_bounds__(BLOCK) k_count_within(const float *__restrict__ dist, int n, TolChunk tc,
                                                        unsigned long long *within) {
    unsigned int c[TOL_CHUNK];
    for (int k = 0; k < TOL_CHUNK; ++k) c[k] = 0;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const float d = dist[i];
        for (int k = 0; k < TOL_CHUNK; ++k) c[k] += (k < tc.n && d <= tc.tol[k]) ? 1u : 0u;
    }
    for (int k = 0; k < TOL_CHUNK; ++k) {
        if (k >= tc.n) break;
        unsigned int v = c[k];
        for (int s = 32; s > 0; s >>= 1) v += (unsigned int)__shfl_xor((int)v, s);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&within[k], (unsigned long long)v);
    }
}

// ---- voxel down-sampling ------------------------------------------------------------------------

// floorf(coordinate / voxel) per axis as a float (an exact integer, possibly huge) and its min/max
__global__ void __launch_bounds__(BLOCK) k_voxel_bounds(const float *__restrict__ xyz, int n, float voxel,
                                                        uint32_t *bounds) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) continue;
        const uint32_t e[3] = {f2ord(floorf(x / voxel)), f2ord(floorf(y / voxel)), f2ord(floorf(z / voxel))};
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], e[a]);
            hi[a] = max(hi[a], e[a]);
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int s = 32; s > 0; s >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], s));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], s));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) {
            if (lo[a] != 0xFFFFFFFFu) atomicMin(&bounds[a], lo[a]);
            if (hi[a] != 0u) atomicMax(&bounds[3 + a], hi[a]);
        }
    }
}

// key = (ix - min_x) << 42 | (iy - min_y) << 21 | (iz - min_z); the caller has checked that every
// span is below 2^21, and the difference of two integer-valued floats that close is exact in double
__global__ void __launch_bounds__(BLOCK) k_voxel_keys(const float *__restrict__ xyz, int n, float voxel, float mx,
                                                      float my, float mz, uint64_t *keys, int *idx) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    uint64_t k = KEY_NONE;
    if (finite3(x, y, z)) {
        const uint64_t ox = (uint64_t)((double)floorf(x / voxel) - (double)mx) & 0x1FFFFFull;
        const uint64_t oy = (uint64_t)((double)floorf(y / voxel) - (double)my) & 0x1FFFFFull;
        const uint64_t oz = (uint64_t)((double)floorf(z / voxel) - (double)mz) & 0x1FFFFFull;
        k = ox << 42 | oy << 21 | oz;
    }
    keys[i] = k;
    idx[i] = i;
}

// the sort is stable and the indices went in ascending, so the first entry of every run of equal
// keys is the lowest input index of that voxel
__global__ void __launch_bounds__(BLOCK) k_voxel_heads(const uint64_t *__restrict__ keys, const int *__restrict__ idx,
                                                       int n, int *flag) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    if (k != KEY_NONE && (i == 0 || keys[i - 1] != k)) flag[idx[i]] = 1;
}

__global__ void __launch_bounds__(BLOCK) k_voxel_compact(const int *__restrict__ flag, const int *__restrict__ pos,
                                                         int n, int *keep, unsigned long long *n_keep) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) keep[pos[i]] = i;
    if (i == n - 1) *n_keep = (unsigned long long)(pos[i] + flag[i]);
}

// ---- z-buffer rendering and visibility ------------------------------------------------------------

constexpr uint64_t PIX_EMPTY = ~0ull;  // above every key: the depth word of a key is below 0x7F800000
constexpr int VIS_CHUNK = 8;           // views per visibility launch (their cameras travel as kernel arguments)

// int(v) as x86-64 cvttss2si, restated from csrc/apd_fusion.hip (trunc_x86).
__device__ __forceinline__ int trunc_x86(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT32_MIN;
    return (int)v;
}

// The render / visibility contract of include/apd_eval.h: project() of csrc/apd_fusion.hip
// (ProjectCamera, APD.cpp:891-900) restated statement for statement, then the rounding its callers
// apply. Returns false for a point that takes no part in the view.
__device__ __forceinline__ bool project_point(const apd_camera &cam, float x, float y, float z, float &d, int &u,
                                              int &v) {
    if (!finite3(x, y, z)) return false;
    const float tx = cam.R[0] * x + cam.R[1] * y + cam.R[2] * z + cam.t[0];
    const float ty = cam.R[3] * x + cam.R[4] * y + cam.R[5] * z + cam.t[1];
    const float tz = cam.R[6] * x + cam.R[7] * y + cam.R[8] * z + cam.t[2];
    d = cam.K[6] * tx + cam.K[7] * ty + cam.K[8] * tz;
    if (!(d > 0.0f && d < __uint_as_float(0x7F800000u))) return false;
    const float px = (cam.K[0] * tx + cam.K[1] * ty + cam.K[2] * tz) / d;
    const float py = (cam.K[3] * tx + cam.K[4] * ty + cam.K[5] * tz) / d;
    u = trunc_x86(px + 0.5f);
    v = trunc_x86(py + 0.5f);
    return true;
}

// One lane per point; the camera is a kernel argument, so its 21 floats come by scalar loads.
// order == nullptr: lane j takes point j; otherwise point order[j] (the Morton order of the cloud).
// Every covered pixel takes the minimum of (bits(d) << 32) | i: d > 0, so its bits order like d, and
// the low word breaks ties towards the lowest point index. The plain load in front of the atomic
// may be stale, but a pixel's key only ever decreases, so a stale value is >= the current one and
// skipping on key >= loaded never drops a key that would have won.
__global__ void __launch_bounds__(BLOCK) k_splat(const float *__restrict__ xyz, const int *__restrict__ order, int n,
                                                 const apd_camera cam, int splat, uint64_t *keys) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const int i = order ? order[j] : j;
    float d;
    int u, v;
    if (!project_point(cam, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], d, u, v)) return;
    const int W = cam.width, H = cam.height;
    // in 64 bits: u or v may be INT32_MIN (covers nothing) or anywhere else in the int range
    const int64_t a0 = max((int64_t)u - splat, (int64_t)0), a1 = min((int64_t)u + splat, (int64_t)W - 1);
    const int64_t b0 = max((int64_t)v - splat, (int64_t)0), b1 = min((int64_t)v + splat, (int64_t)H - 1);
    if (a0 > a1 || b0 > b1) return;
    const uint64_t key = (uint64_t)__float_as_uint(d) << 32 | (uint32_t)i;
    for (int b = (int)b0; b <= (int)b1; ++b)
        for (int a = (int)a0; a <= (int)a1; ++a) {
            uint64_t *p = keys + ((size_t)b * W + a);
            if (key >= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) continue;
            (void)__hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return umin
        }
}

// One lane per pixel: unpack the key plane.
__global__ void __launch_bounds__(BLOCK) k_resolve(const uint64_t *__restrict__ keys, int npix, float *depth,
                                                   int *index) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= npix) return;
    const uint64_t k = keys[p];
    const bool hit = k != PIX_EMPTY;
    depth[p] = hit ? __uint_as_float((uint32_t)(k >> 32)) : 0.0f;
    if (index) index[p] = hit ? (int)(uint32_t)k : -1;
}

struct VisViews {
    apd_camera cam[VIS_CHUNK];
    const float *depth[VIS_CHUNK];
    int n;
};

// One lane per point, a loop over the chunk's views with one gather each, one int32 store per point.
// first: this launch starts the count, otherwise it adds to the earlier chunks'. n_any (last chunk
// only): #{seen > 0}, a ballot and one integer atomic per wave.
__global__ void __launch_bounds__(BLOCK) k_visibility(const float *__restrict__ xyz, int n, const VisViews vv,
                                                      float factor, int first, int *seen,
                                                      unsigned long long *n_any) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    int cnt = 0;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        for (int k = 0; k < vv.n; ++k) {
            const apd_camera &cam = vv.cam[k];
            float d;
            int u, v;
            if (!project_point(cam, x, y, z, d, u, v)) continue;
            if (u < 0 || u >= cam.width || v < 0 || v >= cam.height) continue;
            const float zb = vv.depth[k][(size_t)v * cam.width + u];
            if (zb > 0.0f && d <= zb * factor) ++cnt;
        }
        if (!first) cnt += seen[i];
        seen[i] = cnt;
    }
    if (n_any) {
        const unsigned long long m = __ballot(cnt > 0);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_any, (unsigned long long)__popcll(m));
    }
}

// One lane per point, the views of k_visibility. gap = max over the views that cover the point's
// centre pixel with zb > 0 of zb - d (one fp32 subtraction, never NaN: zb > 0 rules a NaN zb out and
// d is finite), -inf without such a view. first: this launch starts the maximum, otherwise it goes
// on from the earlier chunks'. The maximum does not depend on the order of the views.
__global__ void __launch_bounds__(BLOCK) k_free_gap(const float *__restrict__ xyz, int n, const VisViews vv, int first,
                                                    float *gap) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    float g = first ? __uint_as_float(0xFF800000u) : gap[i];
    for (int k = 0; k < vv.n; ++k) {
        const apd_camera &cam = vv.cam[k];
        float d;
        int u, v;
        if (!project_point(cam, x, y, z, d, u, v)) continue;
        if (u < 0 || u >= cam.width || v < 0 || v >= cam.height) continue;
        const float zb = vv.depth[k][(size_t)v * cam.width + u];
        if (zb > 0.0f) {
            const float e = zb - d;
            if (e > g) g = e;
        }
    }
    gap[i] = g;
}

// ---- voxel scores ---------------------------------------------------------------------------------

// The class of the point at sorted position i for one tolerance, as the summand of the per-voxel
// scan: good << 32 | bad (a run holds fewer than 2^31 points, so neither half carries).
// good: dist <= tol. bad: not good and (no gap given or gap > tol). NaN compares false.
struct ClassOf {
    const int *idx;
    const float *dist;
    const float *gap;  // may be nullptr
    float tol;
    __device__ __forceinline__ uint64_t operator()(int i) const {
        const int j = idx[i];
        const bool good = dist[j] <= tol;
        const bool bad = !good && (gap == nullptr || gap[j] > tol);
        return (uint64_t)good << 32 | (uint64_t)bad;
    }
};

// cnt = the inclusive scan of ClassOf within every run of equal keys, so the last entry of a run
// holds the voxel's (a << 32 | b). Grid-stride over the sorted positions; per lane, then per wave,
// integer sums of a, b, the fixed-point ratio (a << 32) / (a + b) and the number of voxels with
// a + b > 0; the waves of a block meet in LDS, then one integer atomic per block and output (every
// block adds to the same four words, so the atomics are kept few: RATIO_GRID blocks at the most).
// out: good, bad, ratio_sum, voxels.
constexpr int RATIO_GRID = 1024;
__global__ void __launch_bounds__(BLOCK) k_voxel_ratio(const uint64_t *__restrict__ keys,
                                                       const uint64_t *__restrict__ cnt, int n,
                                                       unsigned long long *out) {
    __shared__ unsigned long long part[BLOCK / 64][4];
    unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint64_t k = keys[i];
        if (k == KEY_NONE || (i + 1 < n && keys[i + 1] == k)) continue;
        const uint64_t c = cnt[i], a = c >> 32, b = c & 0xFFFFFFFFull;
        if (a + b == 0) continue;
        acc[0] += a;
        acc[1] += b;
        acc[2] += (a << 32) / (a + b);
        acc[3] += 1;
    }
    for (int q = 0; q < 4; ++q) {
        unsigned long long v = acc[q];
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long v = 0;
        for (int w = 0; w < BLOCK / 64; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(&out[threadIdx.x], v);
    }
}

// ---- crop volume, nearest neighbour with index, registration ----------------------------------------

struct Rows3 {
    double m[12];  // rows 0..2 of a 4x4 transform
};

// The search of k_nearest with the index contract: the minimal computed d2 over the finite targets
// (starting from bound_d2, see k_nearest), the lowest ORIGINAL index among the targets attaining it.
// tidx maps a sorted position to the index given to set_target. best stays INT32_MAX when nothing is
// within the bound; pos is the winner's sorted position. Equal d2 is never pruned (a node is skipped
// only on box_d2 > cur), so every candidate for the tie is seen.
__device__ __forceinline__ void offer_leaf(const Tree &T, const int *__restrict__ tidx, int leaf, float qx, float qy,
                                           float qz, float &cur, int &best, int &pos) {
    const int b = leaf * LEAF, e = min(b + LEAF, T.nf);
    for (int j = b; j < e; ++j) {
        const float d2 = point_d2(qx, qy, qz, T.pts[j]);
        if (d2 <= cur) {
            const int o = tidx[j];
            if (d2 < cur || o < best) {
                cur = d2;
                best = o;
                pos = j;
            }
        }
    }
}

__device__ __forceinline__ void nn_search(const Tree &T, const int *__restrict__ tidx, uint64_t key, float qx, float qy,
                                          float qz, float &cur, int &best, int &pos) {
    int lo = 0, hi = T.nf;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (T.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int leaf0 = min(lo, T.nf - 1) / LEAF;
    offer_leaf(T, tidx, leaf0, qx, qy, qz, cur, best, pos);

    uint32_t st_node[STACK];
    float st_d2[STACK];
    int sp = 0;
    if (T.levels > 1) {
        st_node[0] = (uint32_t)(T.levels - 1) << 27;
        st_d2[0] = 0.0f;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        if (st_d2[sp] > cur) continue;
        const int lvl = (int)(st_node[sp] >> 27), idx = (int)(st_node[sp] & 0x7FFFFFFu);
        const int cl = lvl - 1;
        const int b = idx * FAN, e = min(b + FAN, T.cnt[cl]);
        const float4 *cb = T.boxes + 2 * (size_t)T.off[cl];
        for (int c = b; c < e; ++c) {
            const float bd = box_d2(qx, qy, qz, cb[2 * (size_t)c], cb[2 * (size_t)c + 1]);
            if (bd > cur) continue;
            if (cl == 0) {
                if (c != leaf0) offer_leaf(T, tidx, c, qx, qy, qz, cur, best, pos);
            } else if (sp < STACK) {  // always true (see STACK)
                st_node[sp] = (uint32_t)cl << 27 | (uint32_t)c;
                st_d2[sp] = bd;
                ++sp;
            }
        }
    }
}

// k_nearest with idx: one lane per query, queries in Morton order. dist and idx may be nullptr.
__global__ void __launch_bounds__(BLOCK) k_nearest_idx(const Tree T, const int *__restrict__ tidx, int nq,
                                                       const uint64_t *__restrict__ qkeys,
                                                       const int *__restrict__ qidx, const float *__restrict__ qxyz,
                                                       float bound_d2, float max_dist, float *__restrict__ dist,
                                                       int *__restrict__ idx) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nq) return;
    const int qi = qidx[i];
    const uint64_t key = qkeys[i];
    float r = __uint_as_float(0x7F800000u);
    int ri = -1;
    if (key != KEY_NONE && T.nf > 0) {
        const float qx = qxyz[3 * (size_t)qi], qy = qxyz[3 * (size_t)qi + 1], qz = qxyz[3 * (size_t)qi + 2];
        float cur = bound_d2;
        int best = INT32_MAX, pos = 0;
        nn_search(T, tidx, key, qx, qy, qz, cur, best, pos);
        if (best != INT32_MAX) {
            const float m = sqrtf(cur);
            if (m <= max_dist) {
                r = m;
                ri = best;
            }
        }
    }
    if (dist) dist[qi] = r;
    if (idx) idx[qi] = ri;
}

// One evaluation of a transform, fused: transform, search and the block's tree sum; no q array is
// written. A workgroup of BLOCK lanes owns APD_REG_BLOCK = 4 * BLOCK consecutive source indices and
// takes them in four passes of one index per lane. Per pass the 19 fp64 terms are summed over the
// wave by a butterfly (xor 1, 2, .. 32: IEEE addition commutes, so every lane holds the balanced
// tree's sum over the wave's 64 consecutive indices); lane 0 parks it in LDS slot 4 * pass + wave,
// i.e. in index order. The 16 slots are then summed by the same balanced tree, which makes the whole
// the balanced binary tree over the block's 1024 indices. Indices >= n contribute +0.0 terms.
// Every lane runs every pass to the end: the shuffles need the whole wave.
constexpr int REG_SLOTS = APD_REG_BLOCK / 64;
static_assert(APD_REG_BLOCK == 4 * BLOCK && REG_SLOTS == 16, "the tree below is written for 16 wave sums");
__global__ void __launch_bounds__(BLOCK) k_reg_eval(const Tree T, const int *__restrict__ tidx,
                                                    const uint32_t *__restrict__ bounds,
                                                    const float *__restrict__ xyz, int n, const Rows3 M, float bound_d2,
                                                    float max_corr, double *__restrict__ partials) {
    __shared__ double slot[REG_SLOTS][APD_REG_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int pass = 0; pass < APD_REG_BLOCK / BLOCK; ++pass) {
        const int64_t i = (int64_t)blockIdx.x * APD_REG_BLOCK + pass * BLOCK + threadIdx.x;
        float qx = 0.0f, qy = 0.0f, qz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f, d2 = 0.0f;
        bool fin = false, has = false;
        if (i < n) {
            double p[3];
            apd_reg_xform(M.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], p);
            qx = (float)p[0];
            qy = (float)p[1];
            qz = (float)p[2];
            fin = finite3(qx, qy, qz);
            if (fin && T.nf > 0) {
                const uint64_t key = spread21(quant21(qx, bounds[0], bounds[3])) << 2 |
                                     spread21(quant21(qy, bounds[1], bounds[4])) << 1 |
                                     spread21(quant21(qz, bounds[2], bounds[5]));
                float cur = bound_d2;
                int best = INT32_MAX, pos = 0;
                nn_search(T, tidx, key, qx, qy, qz, cur, best, pos);
                if (best != INT32_MAX && sqrtf(cur) <= max_corr) {
                    const float4 t = T.pts[pos];
                    has = true;
                    tx = t.x;
                    ty = t.y;
                    tz = t.z;
                    d2 = cur;
                }
            }
        }
        double v[APD_REG_SUMS];
        apd_reg_terms(fin, has, qx, qy, qz, tx, ty, tz, d2, v);
        for (int k = 0; k < APD_REG_SUMS; ++k) {
            double a = v[k];
            for (int s = 1; s < 64; s <<= 1) a += __shfl_xor(a, s);
            if (lane == 0) slot[pass * (BLOCK / 64) + wave][k] = a;
        }
    }
    __syncthreads();
    if (threadIdx.x < APD_REG_SUMS) {
        double a[REG_SLOTS];
        for (int w = 0; w < REG_SLOTS; ++w) a[w] = slot[w][threadIdx.x];
        for (int w = REG_SLOTS; w > 1; w >>= 1)
            for (int j = 0; j < w / 2; ++j) a[j] = a[2 * j] + a[2 * j + 1];
        partials[(size_t)blockIdx.x * APD_REG_SUMS + threadIdx.x] = a[0];
    }
}

// The block sums left to right in block order, one lane per sum; no block: +0.0.
__global__ void __launch_bounds__(64) k_reg_fold(const double *__restrict__ partials, int nblocks, double *out) {
    if (threadIdx.x >= APD_REG_SUMS) return;
    double s = 0.0;
    if (nblocks > 0) s = partials[threadIdx.x];
    // the additions are a serial chain; the loads are not, so they are issued eight blocks ahead
    int b = 1;
    for (; b + 8 <= nblocks; b += 8) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = partials[(size_t)(b + k) * APD_REG_SUMS + threadIdx.x];
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nblocks; ++b) s += partials[(size_t)b * APD_REG_SUMS + threadIdx.x];
    out[threadIdx.x] = s;
}

// One lane per point: the crop rule; the polygon is read from memory at wave-uniform addresses.
__global__ void __launch_bounds__(BLOCK) k_crop_flags(const float *__restrict__ xyz, int n, const Rows3 M, int has_T,
                                                      int axis, double axis_min, double axis_max, int m,
                                                      const double *__restrict__ poly, int *flag) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = apd_reg_crop_keep(has_T ? M.m : nullptr, axis, axis_min, axis_max, m, poly, xyz[3 * (size_t)i],
                                xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2])
                  ? 1
                  : 0;
}

__global__ void __launch_bounds__(BLOCK) k_transform(const float *__restrict__ xyz, int n, const Rows3 M, float *out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    apd_reg_xform(M.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], p);
    out[3 * (size_t)i] = (float)p[0];
    out[3 * (size_t)i + 1] = (float)p[1];
    out[3 * (size_t)i + 2] = (float)p[2];
}

// ---- radius thinning, observability mask, half-space, masked statistics ------------------------------

constexpr uint8_t THIN_UNDECIDED = 0, THIN_KEPT = 1, THIN_REMOVED = 2;
constexpr int THIN_RUNS = 9;         // the (y, z) rows around a point's cell, three x cells each
constexpr int THIN_BATCH = 8;        // rounds per read-back once the worklist is small
constexpr int THIN_BATCH_BELOW = 32768;
constexpr uint64_t CELL_MASK = 0x1FFFFFull;

struct ThinGrid {
    double cell;   // 2 * radius
    double lo[3];  // lowest occupied cell per axis
};

// key = cz << 42 | cy << 21 | cx over the occupied cells (apd_dtu_cell; the caller has checked that
// every span is below 2^21): x is the least significant field, so the three x-neighbour cells of a
// (y, z) row are one contiguous run of the sorted array.
__global__ void __launch_bounds__(BLOCK) k_thin_keys(const float *__restrict__ xyz, int n, const ThinGrid g,
                                                     uint64_t *keys, int *idx, unsigned long long *n_finite) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    bool fin = false;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        fin = finite3(x, y, z);
        uint64_t k = KEY_NONE;
        if (fin) {
            const uint64_t cx = (uint64_t)(apd_dtu_cell(x, g.cell) - g.lo[0]) & CELL_MASK;
            const uint64_t cy = (uint64_t)(apd_dtu_cell(y, g.cell) - g.lo[1]) & CELL_MASK;
            const uint64_t cz = (uint64_t)(apd_dtu_cell(z, g.cell) - g.lo[2]) & CELL_MASK;
            k = cz << 42 | cy << 21 | cx;
        }
        keys[i] = k;
        idx[i] = i;
    }
    const unsigned long long m = __ballot(fin);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_finite, (unsigned long long)__popcll(m));
}

// the finite points in cell order, the rank in w (the index half of the priority key is idx_s)
__global__ void __launch_bounds__(BLOCK) k_thin_gather(const float *__restrict__ xyz,
                                                       const uint32_t *__restrict__ rank,
                                                       const int *__restrict__ idx_s, int nf, float4 *pts) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= nf) return;
    const int i = idx_s[p];
    const size_t s = 3 * (size_t)i;
    pts[p] = make_float4(xyz[s], xyz[s + 1], xyz[s + 2], __uint_as_float(rank ? rank[i] : 0u));
}

// first position in keys[0, nf) whose key is >= k
__device__ __forceinline__ int thin_lower_bound(const uint64_t *__restrict__ keys, int lo, int hi, uint64_t k) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The neighbourhood of the point at sorted position p: for each of the 9 (y, z) rows around its cell
// the positions [begin, end) of the cells x - 1 .. x + 1, found once; runs[r * nf + p].
__global__ void __launch_bounds__(BLOCK) k_thin_runs(const uint64_t *__restrict__ keys, int nf, int2 *runs) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= nf) return;
    const uint64_t key = keys[p];
    const int64_t cx = (int64_t)(key & CELL_MASK), cy = (int64_t)(key >> 21 & CELL_MASK), cz = (int64_t)(key >> 42);
    const uint64_t x0 = (uint64_t)max(cx - 1, (int64_t)0), x1 = (uint64_t)min(cx + 1, (int64_t)CELL_MASK);
    for (int r = 0; r < THIN_RUNS; ++r) {
        const int64_t y = cy + r % 3 - 1, z = cz + r / 3 - 1;
        int2 run = make_int2(0, 0);
        if (y >= 0 && z >= 0 && y <= (int64_t)CELL_MASK && z <= (int64_t)CELL_MASK) {
            const uint64_t row = (uint64_t)z << 42 | (uint64_t)y << 21;
            run.x = thin_lower_bound(keys, 0, nf, row | x0);
            run.y = thin_lower_bound(keys, run.x, nf, (row | x1) + 1);
        }
        runs[(size_t)r * nf + p] = run;
    }
}

// One round over the worklist (list == nullptr: positions 0 .. *m_in - 1). Lane = point. A point is
// REMOVED as soon as one close point with a lower key is KEPT, and KEPT as soon as every close point
// with a lower key is REMOVED; both are final, so the state array is updated in place: a read of a
// neighbour's byte that another lane is changing returns UNDECIDED or its final value, and a stale
// UNDECIDED only leaves this point on the worklist for another round. The bytes are read and written
// by relaxed agent-scope atomics (no ordering is needed, only that a byte is read whole).
// The points still undecided are appended to `next` (one integer atomic per wave; their order there
// does not enter the result), their number accumulates in *m_out.
__global__ void __launch_bounds__(BLOCK) k_thin_round(const float4 *__restrict__ pts, const int *__restrict__ idx_s,
                                                      const int2 *__restrict__ runs, int nf, float r2,
                                                      const int *__restrict__ list, const unsigned int *m_in,
                                                      uint8_t *state, int *next, unsigned int *m_out) {
    const unsigned int t = blockIdx.x * BLOCK + threadIdx.x;
    bool pending = false;
    int p = 0;
    if (t < *m_in) {
        p = list ? list[t] : (int)t;
        const float4 a = pts[p];
        const uint32_t ra = __float_as_uint(a.w);
        const int ia = idx_s[p];
        uint8_t verdict = THIN_KEPT;
        for (int r = 0; r < THIN_RUNS && verdict != THIN_REMOVED; ++r) {
            const int2 run = runs[(size_t)r * nf + p];
            for (int j = run.x; j < run.y; ++j) {
                const float4 b = pts[j];
                if (j == p || !apd_dtu_close(a.x, a.y, a.z, b.x, b.y, b.z, r2)) continue;
                const uint32_t rb = __float_as_uint(b.w);
                if (rb > ra || (rb == ra && idx_s[j] > ia)) continue;  // a higher key: no say over p
                const uint8_t s = __hip_atomic_load(state + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (s == THIN_KEPT) {
                    verdict = THIN_REMOVED;
                    break;
                }
                if (s == THIN_UNDECIDED) verdict = THIN_UNDECIDED;
            }
        }
        if (verdict != THIN_UNDECIDED)
            __hip_atomic_store(state + p, verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            pending = true;
    }
    const unsigned long long m = __ballot(pending);
    if (m) {  // wave-uniform
        const int lane = threadIdx.x & 63;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(m_out, (unsigned int)__popcll(m));
        base = (unsigned int)__shfl((int)base, 0);
        if (pending) next[base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = p;
    }
}

__global__ void __launch_bounds__(BLOCK) k_thin_flags(const uint8_t *__restrict__ state, const int *__restrict__ idx_s,
                                                      int nf, int *flag) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= nf) return;
    if (state[p] == THIN_KEPT) flag[idx_s[p]] = 1;
}

__global__ void __launch_bounds__(BLOCK) k_obs_mask(const float *__restrict__ xyz, int n, const apd_dtu_mask_geom g,
                                                    const uint8_t *__restrict__ mask, uint8_t *inside) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    inside[i] = apd_dtu_inside(g, mask, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) ? 1 : 0;
}

struct Plane4 {
    double P[4];
};
__global__ void __launch_bounds__(BLOCK) k_half_space(const float *__restrict__ xyz, int n, const Plane4 pl,
                                                      uint8_t *above) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    above[i] = apd_dtu_above(pl.P, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) ? 1 : 0;
}

// The selection, its count, the sort keys and the block sums of the masked statistics. A workgroup
// owns APD_REG_BLOCK consecutive indices in four passes, as k_reg_eval does, with one term per index:
// the butterfly over a wave, the wave sums parked in index order, the same tree over the 16 slots.
// keys[i] = the ordered image of a selected distance, else 0xFFFFFFFF (the image of no selected value:
// only a NaN maps there), so the selected values are the first `count` entries of the sorted keys.
__global__ void __launch_bounds__(BLOCK) k_stats_block(const float *__restrict__ dist,
                                                       const uint8_t *__restrict__ flag, int n, float limit,
                                                       double *__restrict__ partials, uint32_t *keys,
                                                       unsigned long long *count) {
    __shared__ double slot[REG_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int pass = 0; pass < APD_REG_BLOCK / BLOCK; ++pass) {
        const int64_t i = (int64_t)blockIdx.x * APD_REG_BLOCK + pass * BLOCK + threadIdx.x;
        bool sel = false;
        double a = 0.0;
        if (i < n) {
            const float d = dist[i];
            sel = apd_dtu_selected(d, !flag || flag[i] != 0, limit);
            if (sel) a = (double)d;
            keys[i] = sel ? apd_dtu_ord(d) : 0xFFFFFFFFu;
        }
        for (int s = 1; s < 64; s <<= 1) a += __shfl_xor(a, s);
        const unsigned long long m = __ballot(sel);
        if (lane == 0) {
            slot[pass * (BLOCK / 64) + wave] = a;
            if (m) atomicAdd(count, (unsigned long long)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a[REG_SLOTS];
        for (int w = 0; w < REG_SLOTS; ++w) a[w] = slot[w];
        for (int w = REG_SLOTS; w > 1; w >>= 1)
            for (int j = 0; j < w / 2; ++j) a[j] = a[2 * j] + a[2 * j + 1];
        partials[blockIdx.x] = a[0];
    }
}

// the block sums left to right from block 0's sum; no block: +0.0
__global__ void __launch_bounds__(64) k_stats_fold(const double *__restrict__ partials, int nblocks, double *out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    if (nblocks > 0) s = partials[0];
    int b = 1;
    for (; b + 8 <= nblocks; b += 8) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = partials[b + k];
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nblocks; ++b) s += partials[b];
    out[0] = s;
}

inline int grid_for(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }
inline int grid_capped(int64_t n) { return (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 4096); }

}  // namespace

struct apd_eval_ctx : DevCtx {
    apd_eval_ctx() : DevCtx("apd_eval") {}
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // target
    DevBuf t_xyz, t_keys, t_keys_s, t_idx, t_idx_s, t_pts, t_boxes;
    // query / voxel working set
    DevBuf q_xyz, q_keys, q_keys_s, q_idx, q_idx_s, q_dist, q_aux;
    DevBuf sort_tmp, small;  // small: bounds (6 u32) at 0, counters (u64) from byte 64
    Tree tree{};
    bool has_target = false;
    double build_ms = 0.0, query_ms = 0.0, voxel_ms = 0.0;
    // render / visibility: the key plane of one view, staging for its outputs (render) or for the
    // depth maps of one chunk of views (visibility), and the cloud's own bounds for the Morton order
    DevBuf r_keys, r_depth, r_index, r_small;
    bool render_morton = false;  // APD_EVAL_RENDER_ORDER=input|morton (input measured faster)
    double render_ms = 0.0, visibility_ms = 0.0;
    // free gap / voxel scores: device copies of dist and gap, the per-run scan of one tolerance and
    // the four sums of every tolerance
    DevBuf s_dist, s_gap, s_cnt, s_out;
    double free_gap_ms = 0.0, scores_ms = 0.0;
    // crop / nearest with index / transform / registration: the polygon, the transformed cloud, the
    // per-block sums and the 19 folded sums; a third event splits the evaluation from the fold
    DevBuf c_poly, x_out, g_part, g_sums, n_idx;
    hipEvent_t ev2 = nullptr;
    double reg_eval_ms = 0.0, reg_fold_ms = 0.0, reg_solve_ms = 0.0, crop_ms = 0.0, transform_ms = 0.0;
    int reg_evaluations = 0;
    // radius thinning: the points in cell order with their ranks, the 9 neighbour runs of every point,
    // a byte of state each, the two worklists, the uploaded ranks and the per-round counters
    DevBuf th_pts, th_runs, th_state, th_list0, th_list1, th_rank, th_small;
    double thin_sort_ms = 0.0, thin_rounds_ms = 0.0;
    int thin_rounds = 0;
    // observability mask (kept while the caller gives the same pointer and dims), the flags of a call,
    // the statistics' block sums and results
    DevBuf m_mask, d_flag, st_part, st_out;
    const void *mask_src = nullptr;
    int32_t mask_dims[3] = {0, 0, 0};
    double mask_ms = 0.0, half_space_ms = 0.0, stats_ms = 0.0;
};

static int check_n(apd_eval_ctx *ctx, const char *what, int64_t n, const void *p) {
    if (n < 0 || n > (int64_t)INT32_MAX) {
        ctx->err = std::string(what) + ": point count out of range";
        return APD_EINVAL;
    }
    if (n > 0 && !p) {
        ctx->err = std::string(what) + ": NULL point array";
        return APD_EINVAL;
    }
    return APD_OK;
}

// keys/idx -> keys_s/idx_s, stable, all 64 bits
static int sort_pairs(apd_eval_ctx *ctx, DevBuf &keys, DevBuf &keys_s, DevBuf &idx, DevBuf &idx_s, int n) {
    size_t tb = 0;
    HIP_OK(ctx, rocprim::radix_sort_pairs(nullptr, tb, (uint64_t *)keys.p, (uint64_t *)keys_s.p, (int *)idx.p,
                                         (int *)idx_s.p, (size_t)n, 0, 64, ctx->stream));
    int st = grow(ctx, ctx->sort_tmp, tb);
    if (st) return st;
    HIP_OK(ctx, rocprim::radix_sort_pairs(ctx->sort_tmp.p, tb, (uint64_t *)keys.p, (uint64_t *)keys_s.p, (int *)idx.p,
                                         (int *)idx_s.p, (size_t)n, 0, 64, ctx->stream));
    return APD_OK;
}

// the largest float b with sqrtf(b) <= md (md >= 0, not NaN); +inf when there is no cut-off
static float d2_bound(float md) {
    const float inf = std::numeric_limits<float>::infinity();
    if (md == inf) return inf;
    float b = (float)((double)md * (double)md);
    if (b == inf) b = std::numeric_limits<float>::max();
    while (b > 0.0f && sqrtf(b) > md) b = std::nextafterf(b, 0.0f);
    for (;;) {
        const float nx = std::nextafterf(b, inf);
        if (nx == inf || sqrtf(nx) > md) break;
        b = nx;
    }
    return b;
}

// The voxel keys of the n points in q_xyz, sorted: q_keys_s / q_idx_s (stable, so equal keys keep
// ascending input indices; non-finite points sort last under KEY_NONE). bounds: 6 words of device
// scratch. none = true (and nothing sorted) when no point is finite. Drains the stream once.
static int voxel_sorted_keys(apd_eval_ctx *ctx, const char *what, int n, float voxel, uint32_t *bounds, bool &none) {
    hipStream_t s = ctx->stream;
    int st;
    HIP_OK(ctx, hipMemsetAsync(bounds, 0xFF, 12, s));
    HIP_OK(ctx, hipMemsetAsync(bounds + 3, 0, 12, s));
    hipLaunchKernelGGL(k_voxel_bounds, dim3(grid_capped(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, voxel,
                       bounds);
    HIP_OK(ctx, hipGetLastError());
    uint32_t hb[6];
    HIP_OK(ctx, hipMemcpyAsync(hb, bounds, 24, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    none = hb[0] == 0xFFFFFFFFu;
    if (none) return APD_OK;
    float mn[3];
    for (int a = 0; a < 3; ++a) {
        auto dec = [](uint32_t u) {
            const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
            float f;
            memcpy(&f, &b, 4);
            return f;
        };
        mn[a] = dec(hb[a]);
        const double span = (double)dec(hb[3 + a]) - (double)mn[a];
        if (!(span < 2097152.0)) {
            ctx->err = std::string(what) + ": an axis spans more than 2^21 voxels";
            return APD_EINVAL;
        }
    }
    hipLaunchKernelGGL(k_voxel_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, voxel,
                       mn[0], mn[1], mn[2], (uint64_t *)ctx->q_keys.p, (int *)ctx->q_idx.p);
    HIP_OK(ctx, hipGetLastError());
    if ((st = sort_pairs(ctx, ctx->q_keys, ctx->q_keys_s, ctx->q_idx, ctx->q_idx_s, n))) return st;
    return APD_OK;
}

extern "C" {

apd_eval_ctx *apd_eval_create(int32_t device) {
    auto *ctx = open_ctx<apd_eval_ctx>(device);
    if (!ctx) return nullptr;
    if (const char *e = getenv("APD_EVAL_RENDER_ORDER")) ctx->render_morton = strcmp(e, "morton") == 0;
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreate(&ctx->ev2) != hipSuccess) {
        apd_eval_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void apd_eval_destroy(apd_eval_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // the buffers with it
}

const char *apd_eval_last_error(const apd_eval_ctx *ctx) {
    return ctx ? ctx->err.c_str() : "apd_eval_create failed (no such HIP device)";
}

int32_t apd_eval_set_target(apd_eval_ctx *ctx, int64_t n64, const float *xyz) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_set_target", n64, xyz);
    if (st) return st;
    const int n = (int)n64;
    ctx->build_ms = 0.0;
    if (n == 0) {  // an empty target is a target: every distance is +inf
        ctx->tree = Tree{};
        ctx->has_target = true;
        return APD_OK;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    ctx->has_target = false;
    if ((st = grow(ctx, ctx->t_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->t_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->t_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->t_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->t_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->small, 256)))
        return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->t_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    uint32_t *bounds = (uint32_t *)ctx->small.p;
    unsigned long long *counter = (unsigned long long *)((char *)ctx->small.p + 64);
    HIP_OK(ctx, hipMemsetAsync(bounds, 0xFF, 12, s));
    HIP_OK(ctx, hipMemsetAsync(bounds + 3, 0, 12, s));
    HIP_OK(ctx, hipMemsetAsync(counter, 0, 8, s));
    hipLaunchKernelGGL(k_bounds, dim3(grid_capped(n)), dim3(BLOCK), 0, s, (const float *)ctx->t_xyz.p, n, bounds);
    hipLaunchKernelGGL(k_morton_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->t_xyz.p, n, bounds,
                       (uint64_t *)ctx->t_keys.p, (int *)ctx->t_idx.p, counter);
    HIP_OK(ctx, hipGetLastError());
    if ((st = sort_pairs(ctx, ctx->t_keys, ctx->t_keys_s, ctx->t_idx, ctx->t_idx_s, n))) return st;
    unsigned long long nf64 = 0;
    HIP_OK(ctx, hipMemcpyAsync(&nf64, counter, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const int nf = (int)nf64;
    Tree T{};
    T.nf = nf;
    if (nf > 0) {
        int total = 0, c = (nf + LEAF - 1) / LEAF;
        for (;;) {
            T.off[T.levels] = total;
            T.cnt[T.levels] = c;
            total += c;
            ++T.levels;
            if (c == 1) break;
            c = (c + FAN - 1) / FAN;
        }
        if ((st = grow(ctx, ctx->t_pts, (size_t)nf * 16)) || (st = grow(ctx, ctx->t_boxes, (size_t)total * 32)))
            return st;
        float4 *boxes = (float4 *)ctx->t_boxes.p;
        hipLaunchKernelGGL(k_gather_points, dim3(grid_for(nf)), dim3(BLOCK), 0, s, (const float *)ctx->t_xyz.p,
                           (const int *)ctx->t_idx_s.p, nf, (float4 *)ctx->t_pts.p);
        hipLaunchKernelGGL(k_leaf_boxes, dim3(grid_for(T.cnt[0])), dim3(BLOCK), 0, s, (const float4 *)ctx->t_pts.p, nf,
                           T.cnt[0], boxes);
        for (int l = 1; l < T.levels; ++l)
            hipLaunchKernelGGL(k_upper_boxes, dim3(grid_for(T.cnt[l])), dim3(BLOCK), 0, s,
                               (const float4 *)(boxes + 2 * (size_t)T.off[l - 1]), T.cnt[l - 1], T.cnt[l],
                               boxes + 2 * (size_t)T.off[l]);
        HIP_OK(ctx, hipGetLastError());
        T.pts = (const float4 *)ctx->t_pts.p;
        T.boxes = boxes;
        T.keys = (const uint64_t *)ctx->t_keys_s.p;
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ctx->build_ms))) return st;
    ctx->tree = T;
    ctx->has_target = true;
    return APD_OK;
}

int32_t apd_eval_distances(apd_eval_ctx *ctx, int64_t n64, const float *xyz, float max_dist, float *dist,
                           int32_t num_tol, const float *tol, int64_t *within) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_distances", n64, xyz);
    if (st) return st;
    if (!(max_dist >= 0.0f)) {
        ctx->err = "apd_eval_distances: max_dist is negative or NaN";
        return APD_EINVAL;
    }
    if (num_tol < 0 || (num_tol > 0 && !tol)) {
        ctx->err = "apd_eval_distances: bad tolerance list";
        return APD_EINVAL;
    }
    if (!ctx->has_target) {
        ctx->err = "apd_eval_distances: no target set";
        return APD_ESTATE;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    std::vector<float> tols((size_t)num_tol);
    if (num_tol > 0) HIP_OK(ctx, hipMemcpy(tols.data(), tol, (size_t)num_tol * 4, hipMemcpyDefault));
    for (float t : tols)
        if (!(t >= 0.0f) || t > max_dist) {
            ctx->err = "apd_eval_distances: a tolerance is negative, NaN or above max_dist";
            return APD_EINVAL;
        }
    const int n = (int)n64;
    ctx->query_ms = 0.0;
    std::vector<unsigned long long> counts((size_t)num_tol, 0ull);
    if (n == 0) {
        if (within && num_tol > 0)
            HIP_OK(ctx, hipMemcpy(within, counts.data(), (size_t)num_tol * 8, hipMemcpyDefault));
        return APD_OK;
    }
    const int ncnt = within ? num_tol : 0;
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_aux, (size_t)std::max(ncnt, 1) * 8)) || (st = grow(ctx, ctx->small, 256)))
        return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    // queries are keyed over the TARGET's bounding box, still in `small` from set_target (an all-
    // non-finite or empty target leaves no usable box: every key is then 0 or NONE, which is fine)
    const uint32_t *bounds = (const uint32_t *)ctx->small.p;
    hipLaunchKernelGGL(k_morton_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, bounds,
                       (uint64_t *)ctx->q_keys.p, (int *)ctx->q_idx.p, (unsigned long long *)nullptr);
    HIP_OK(ctx, hipGetLastError());
    if ((st = sort_pairs(ctx, ctx->q_keys, ctx->q_keys_s, ctx->q_idx, ctx->q_idx_s, n))) return st;
    hipLaunchKernelGGL(k_nearest, dim3(grid_for(n)), dim3(BLOCK), 0, s, ctx->tree, n,
                       (const uint64_t *)ctx->q_keys_s.p, (const int *)ctx->q_idx_s.p, (const float *)ctx->q_xyz.p,
                       d2_bound(max_dist), max_dist, (float *)ctx->q_dist.p);
    HIP_OK(ctx, hipGetLastError());
    if (ncnt > 0) {
        HIP_OK(ctx, hipMemsetAsync(ctx->q_aux.p, 0, (size_t)ncnt * 8, s));
        for (int k0 = 0; k0 < ncnt; k0 += TOL_CHUNK) {
            TolChunk tc{};
            tc.n = std::min(TOL_CHUNK, ncnt - k0);
            for (int k = 0; k < tc.n; ++k) tc.tol[k] = tols[(size_t)(k0 + k)];
            hipLaunchKernelGGL(k_count_within, dim3(grid_capped(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_dist.p,
                               n, tc, (unsigned long long *)ctx->q_aux.p + k0);
        }
        HIP_OK(ctx, hipGetLastError());
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    if (dist) HIP_OK(ctx, hipMemcpyAsync(dist, ctx->q_dist.p, (size_t)n * 4, hipMemcpyDefault, s));
    if (ncnt > 0) HIP_OK(ctx, hipMemcpyAsync(within, ctx->q_aux.p, (size_t)ncnt * 8, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->query_ms);
}

int32_t apd_eval_voxel_downsample(apd_eval_ctx *ctx, int64_t n64, const float *xyz, float voxel, int32_t *keep_idx,
                                  int64_t *n_keep) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_voxel_downsample", n64, xyz);
    if (st) return st;
    if (!(voxel > 0.0f) || !std::isfinite(voxel)) {
        ctx->err = "apd_eval_voxel_downsample: voxel must be positive and finite";
        return APD_EINVAL;
    }
    if (!n_keep || (n64 > 0 && !keep_idx)) {
        ctx->err = "apd_eval_voxel_downsample: NULL output";
        return APD_EINVAL;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    ctx->voxel_ms = 0.0;
    unsigned long long kept = 0;
    if (n == 0) {
        HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
        return APD_OK;
    }
    // q_dist holds the head flags, q_aux their exclusive scan, q_keys (reused) the kept indices
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_aux, 128 + (size_t)n * 4)))
        return st;
    // q_aux: bounds at byte 0, the kept count at byte 64, the scan from byte 128. Its own scratch for the bounds: `small` keeps the target's box for apd_eval_distances
    uint32_t *bounds = (uint32_t *)ctx->q_aux.p;
    unsigned long long *counter = (unsigned long long *)((char *)ctx->q_aux.p + 64);
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    bool none = false;
    if ((st = voxel_sorted_keys(ctx, "apd_eval_voxel_downsample", n, voxel, bounds, none))) return st;
    if (none) {  // no finite point
        HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
        return APD_OK;
    }
    int *flag = (int *)ctx->q_dist.p, *pos = (int *)ctx->q_aux.p + 32, *keep = (int *)ctx->q_keys.p;
    HIP_OK(ctx, hipMemsetAsync(flag, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(k_voxel_heads, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t *)ctx->q_keys_s.p,
                       (const int *)ctx->q_idx_s.p, n, flag);
    HIP_OK(ctx, hipGetLastError());
    size_t tb = 0;
    HIP_OK(ctx, rocprim::exclusive_scan(nullptr, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    if ((st = grow(ctx, ctx->sort_tmp, tb))) return st;
    HIP_OK(ctx, rocprim::exclusive_scan(ctx->sort_tmp.p, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(k_voxel_compact, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const int *)flag, (const int *)pos, n,
                       keep, counter);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(&kept, counter, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if (kept > 0) HIP_OK(ctx, hipMemcpy(keep_idx, keep, (size_t)kept * 4, hipMemcpyDefault));
    HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->voxel_ms);
}

int32_t apd_eval_get_timing(apd_eval_ctx *ctx, double *build_ms, double *query_ms, double *voxel_ms) {
    if (!ctx) return APD_EINVAL;
    if (build_ms) *build_ms = ctx->build_ms;
    if (query_ms) *query_ms = ctx->query_ms;
    if (voxel_ms) *voxel_ms = ctx->voxel_ms;
    return APD_OK;
}

static int check_views(apd_eval_ctx *ctx, const char *what, int32_t num_views, const apd_camera *cams) {
    if (num_views < 0 || (num_views > 0 && !cams)) {
        ctx->err = std::string(what) + ": bad view list";
        return APD_EINVAL;
    }
    for (int v = 0; v < num_views; ++v)
        if (cams[v].width < 1 || cams[v].height < 1 ||
            (int64_t)cams[v].width * (int64_t)cams[v].height > ((int64_t)1 << 28)) {
            ctx->err = std::string(what) + ": view " + std::to_string(v) + " has a size outside 1..2^28 pixels";
            return APD_EINVAL;
        }
    return APD_OK;
}

int32_t apd_eval_render_depth(apd_eval_ctx *ctx, int64_t n64, const float *xyz, int32_t num_views,
                              const apd_camera *cams, int32_t splat, float *const *depth, int32_t *const *index) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_render_depth", n64, xyz);
    if (st || (st = check_views(ctx, "apd_eval_render_depth", num_views, cams))) return st;
    if (splat < 0 || splat > 16) {
        ctx->err = "apd_eval_render_depth: splat outside 0..16";
        return APD_EINVAL;
    }
    if (num_views > 0 && !depth) {
        ctx->err = "apd_eval_render_depth: NULL depth map list";
        return APD_EINVAL;
    }
    for (int v = 0; v < num_views; ++v)
        if (!depth[v]) {
            ctx->err = "apd_eval_render_depth: NULL depth map";
            return APD_EINVAL;
        }
    ctx->render_ms = 0.0;
    if (num_views == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    size_t max_pix = 0;
    bool any_index = false;
    for (int v = 0; v < num_views; ++v) {
        max_pix = std::max(max_pix, (size_t)cams[v].width * (size_t)cams[v].height);
        any_index = any_index || (index && index[v]);
    }
    if ((st = grow(ctx, ctx->r_keys, max_pix * 8)) || (st = grow(ctx, ctx->r_depth, max_pix * 4)) ||
        (any_index && (st = grow(ctx, ctx->r_index, max_pix * 4))))
        return st;
    hipStream_t s = ctx->stream;
    const int *order = nullptr;
    double ms = 0.0, total = 0.0;
    if (n > 0) {
        if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12))) return st;
        HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
        if (ctx->render_morton) {
            // the key-and-sort path of set_target over the cloud's own box; `small` keeps the target's
            if ((st = grow(ctx, ctx->q_keys, (size_t)n * 8)) || (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) ||
                (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) || (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) ||
                (st = grow(ctx, ctx->r_small, 64)))
                return st;
            uint32_t *bounds = (uint32_t *)ctx->r_small.p;
            HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
            HIP_OK(ctx, hipMemsetAsync(bounds, 0xFF, 12, s));
            HIP_OK(ctx, hipMemsetAsync(bounds + 3, 0, 12, s));
            hipLaunchKernelGGL(k_bounds, dim3(grid_capped(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, bounds);
            hipLaunchKernelGGL(k_morton_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n,
                               (const uint32_t *)bounds, (uint64_t *)ctx->q_keys.p, (int *)ctx->q_idx.p,
                               (unsigned long long *)nullptr);
            HIP_OK(ctx, hipGetLastError());
            if ((st = sort_pairs(ctx, ctx->q_keys, ctx->q_keys_s, ctx->q_idx, ctx->q_idx_s, n))) return st;
            HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ms))) return st;
            total += ms;
            order = (const int *)ctx->q_idx_s.p;
        }
    }
    for (int v = 0; v < num_views; ++v) {
        const int npix = cams[v].width * cams[v].height;
        int *idx_out = (index && index[v]) ? (int *)ctx->r_index.p : nullptr;
        HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
        HIP_OK(ctx, hipMemsetAsync(ctx->r_keys.p, 0xFF, (size_t)npix * 8, s));
        if (n > 0)
            hipLaunchKernelGGL(k_splat, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, order, n,
                               cams[v], (int)splat, (uint64_t *)ctx->r_keys.p);
        hipLaunchKernelGGL(k_resolve, dim3(grid_for(npix)), dim3(BLOCK), 0, s, (const uint64_t *)ctx->r_keys.p, npix,
                           (float *)ctx->r_depth.p, idx_out);
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
        HIP_OK(ctx, hipMemcpyAsync(depth[v], ctx->r_depth.p, (size_t)npix * 4, hipMemcpyDefault, s));
        if (idx_out) HIP_OK(ctx, hipMemcpyAsync(index[v], idx_out, (size_t)npix * 4, hipMemcpyDefault, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ms))) return st;
        total += ms;
    }
    ctx->render_ms = total;
    return APD_OK;
}

int32_t apd_eval_visibility(apd_eval_ctx *ctx, int64_t n64, const float *xyz, int32_t num_views,
                            const apd_camera *cams, const float *const *depth, float rel_tol, int32_t *seen,
                            int64_t *n_visible_any) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_visibility", n64, xyz);
    if (st || (st = check_views(ctx, "apd_eval_visibility", num_views, cams))) return st;
    if (!(rel_tol >= 0.0f) || !std::isfinite(rel_tol)) {
        ctx->err = "apd_eval_visibility: rel_tol is negative or not finite";
        return APD_EINVAL;
    }
    if ((n64 > 0 && !seen) || (num_views > 0 && !depth)) {
        ctx->err = "apd_eval_visibility: NULL seen array or depth map list";
        return APD_EINVAL;
    }
    for (int v = 0; v < num_views; ++v)
        if (!depth[v]) {
            ctx->err = "apd_eval_visibility: NULL depth map";
            return APD_EINVAL;
        }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    ctx->visibility_ms = 0.0;
    unsigned long long any = 0;
    if (n == 0) {
        if (n_visible_any) HIP_OK(ctx, hipMemcpy(n_visible_any, &any, 8, hipMemcpyDefault));
        return APD_OK;
    }
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->r_small, 64)))
        return st;
    hipStream_t s = ctx->stream;
    int *d_seen = (int *)ctx->q_dist.p;
    unsigned long long *counter = (unsigned long long *)((char *)ctx->r_small.p + 32);
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipMemsetAsync(counter, 0, 8, s));
    if (num_views == 0) HIP_OK(ctx, hipMemsetAsync(d_seen, 0, (size_t)n * 4, s));
    const float factor = 1.0f + rel_tol;  // one fp32 addition, made once
    double ms = 0.0, total = 0.0;
    for (int v0 = 0; v0 < num_views; v0 += VIS_CHUNK) {
        VisViews vv{};
        vv.n = std::min(VIS_CHUNK, num_views - v0);
        size_t bytes = 0;
        for (int k = 0; k < vv.n; ++k) bytes += (size_t)cams[v0 + k].width * (size_t)cams[v0 + k].height * 4;
        if ((st = grow(ctx, ctx->r_depth, bytes))) return st;
        size_t off = 0;
        for (int k = 0; k < vv.n; ++k) {
            const size_t b = (size_t)cams[v0 + k].width * (size_t)cams[v0 + k].height * 4;
            vv.cam[k] = cams[v0 + k];
            vv.depth[k] = (const float *)((char *)ctx->r_depth.p + off);
            HIP_OK(ctx, hipMemcpyAsync((char *)ctx->r_depth.p + off, depth[v0 + k], b, hipMemcpyDefault, s));
            off += b;
        }
        const bool last = v0 + VIS_CHUNK >= num_views;
        HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
        hipLaunchKernelGGL(k_visibility, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, vv, factor,
                           v0 == 0 ? 1 : 0, d_seen, last ? counter : (unsigned long long *)nullptr);
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
        HIP_OK(ctx, hipStreamSynchronize(s));  // the next chunk reuses the staging buffer and the events
        if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ms))) return st;
        total += ms;
    }
    HIP_OK(ctx, hipMemcpyAsync(seen, d_seen, (size_t)n * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipMemcpyAsync(&any, counter, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if (n_visible_any) HIP_OK(ctx, hipMemcpy(n_visible_any, &any, 8, hipMemcpyDefault));
    ctx->visibility_ms = total;
    return APD_OK;
}

int32_t apd_eval_get_render_timing(apd_eval_ctx *ctx, double *render_ms, double *visibility_ms) {
    if (!ctx) return APD_EINVAL;
    if (render_ms) *render_ms = ctx->render_ms;
    if (visibility_ms) *visibility_ms = ctx->visibility_ms;
    return APD_OK;
}

int32_t apd_eval_cube_cameras(const float origin[3], int32_t size, apd_camera cams[6]) {
    if (!origin || !cams || size < 2 || size > 16384) return APD_EINVAL;
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return APD_EINVAL;
    // rows (right, down, forward) of the faces +X, -X, +Y, -Y, +Z, -Z; every determinant is +1
    static const float kR[6][9] = {{0, 0, -1, 0, 1, 0, 1, 0, 0},  {0, 0, 1, 0, 1, 0, -1, 0, 0},
                                   {1, 0, 0, 0, 0, -1, 0, 1, 0},  {1, 0, 0, 0, 0, 1, 0, -1, 0},
                                   {1, 0, 0, 0, 1, 0, 0, 0, 1},   {-1, 0, 0, 0, 1, 0, 0, 0, -1}};
    const float f = 0.5f * (float)size;  // exact
    for (int k = 0; k < 6; ++k) {
        apd_camera c{};
        memcpy(c.R, kR[k], sizeof c.R);
        for (int r = 0; r < 3; ++r)  // exact: one entry of a row is +-1, the others are 0
            c.t[r] = -(c.R[3 * r] * origin[0] + c.R[3 * r + 1] * origin[1] + c.R[3 * r + 2] * origin[2]);
        c.K[0] = c.K[4] = f;
        c.K[2] = c.K[5] = f - 0.5f;
        c.K[8] = 1.0f;
        c.width = c.height = size;
        cams[k] = c;
    }
    return APD_OK;
}

int32_t apd_eval_free_gap(apd_eval_ctx *ctx, int64_t n64, const float *xyz, int32_t num_views, const apd_camera *cams,
                          const float *const *depth, float *gap) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_free_gap", n64, xyz);
    if (st || (st = check_views(ctx, "apd_eval_free_gap", num_views, cams))) return st;
    if ((n64 > 0 && !gap) || (num_views > 0 && !depth)) {
        ctx->err = "apd_eval_free_gap: NULL gap array or depth map list";
        return APD_EINVAL;
    }
    for (int v = 0; v < num_views; ++v)
        if (!depth[v]) {
            ctx->err = "apd_eval_free_gap: NULL depth map";
            return APD_EINVAL;
        }
    ctx->free_gap_ms = 0.0;
    const int n = (int)n64;
    if (n == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4))) return st;
    hipStream_t s = ctx->stream;
    float *d_gap = (float *)ctx->q_dist.p;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    double ms = 0.0, total = 0.0;
    int v0 = 0;
    do {  // at least once: without views the kernel still writes -inf
        VisViews vv{};
        vv.n = std::min(VIS_CHUNK, num_views - v0);
        size_t bytes = 0;
        for (int k = 0; k < vv.n; ++k) bytes += (size_t)cams[v0 + k].width * (size_t)cams[v0 + k].height * 4;
        if ((st = grow(ctx, ctx->r_depth, bytes))) return st;
        size_t off = 0;
        for (int k = 0; k < vv.n; ++k) {
            const size_t b = (size_t)cams[v0 + k].width * (size_t)cams[v0 + k].height * 4;
            vv.cam[k] = cams[v0 + k];
            vv.depth[k] = (const float *)((char *)ctx->r_depth.p + off);
            HIP_OK(ctx, hipMemcpyAsync((char *)ctx->r_depth.p + off, depth[v0 + k], b, hipMemcpyDefault, s));
            off += b;
        }
        HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
        hipLaunchKernelGGL(k_free_gap, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, vv,
                           v0 == 0 ? 1 : 0, d_gap);
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
        HIP_OK(ctx, hipStreamSynchronize(s));  // the next chunk reuses the staging buffer and the events
        if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ms))) return st;
        total += ms;
        v0 += VIS_CHUNK;
    } while (v0 < num_views);
    HIP_OK(ctx, hipMemcpyAsync(gap, d_gap, (size_t)n * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    ctx->free_gap_ms = total;
    return APD_OK;
}

int32_t apd_eval_voxel_scores(apd_eval_ctx *ctx, int64_t n64, const float *xyz, float voxel, const float *dist,
                              const float *gap, int32_t num_tol, const float *tol, int64_t *good, int64_t *bad,
                              uint64_t *ratio_sum, int64_t *voxels) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_voxel_scores", n64, xyz);
    if (st) return st;
    if (!(voxel > 0.0f) || !std::isfinite(voxel)) {
        ctx->err = "apd_eval_voxel_scores: voxel must be positive and finite";
        return APD_EINVAL;
    }
    if (n64 > 0 && !dist) {
        ctx->err = "apd_eval_voxel_scores: NULL dist array";
        return APD_EINVAL;
    }
    if (num_tol < 0 || (num_tol > 0 && !tol)) {
        ctx->err = "apd_eval_voxel_scores: bad tolerance list";
        return APD_EINVAL;
    }
    if (num_tol > 0 && (!good || !bad || !ratio_sum || !voxels)) {
        ctx->err = "apd_eval_voxel_scores: NULL output";
        return APD_EINVAL;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    std::vector<float> tols((size_t)num_tol);
    if (num_tol > 0) HIP_OK(ctx, hipMemcpy(tols.data(), tol, (size_t)num_tol * 4, hipMemcpyDefault));
    for (float t : tols)
        if (!(t >= 0.0f)) {
            ctx->err = "apd_eval_voxel_scores: a tolerance is negative or NaN";
            return APD_EINVAL;
        }
    const int n = (int)n64;
    ctx->scores_ms = 0.0;
    // host copy of the sums, tolerance-major: good, bad, ratio_sum, voxels
    std::vector<unsigned long long> sums((size_t)num_tol * 4, 0ull);
    auto deliver = [&]() -> int {
        std::vector<unsigned long long> col((size_t)num_tol);
        void *const outs[4] = {good, bad, ratio_sum, voxels};
        for (int q = 0; q < 4 && num_tol > 0; ++q) {
            for (int k = 0; k < num_tol; ++k) col[(size_t)k] = sums[(size_t)k * 4 + q];
            HIP_OK(ctx, hipMemcpy(outs[q], col.data(), (size_t)num_tol * 8, hipMemcpyDefault));
        }
        return APD_OK;
    };
    if (n == 0) return deliver();
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->q_aux, 128)) ||
        (st = grow(ctx, ctx->s_dist, (size_t)n * 4)) || (gap && (st = grow(ctx, ctx->s_gap, (size_t)n * 4))) ||
        (st = grow(ctx, ctx->s_cnt, (size_t)n * 8)) || (st = grow(ctx, ctx->s_out, (size_t)std::max(num_tol, 1) * 32)))
        return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->s_dist.p, dist, (size_t)n * 4, hipMemcpyDefault, s));
    if (gap) HIP_OK(ctx, hipMemcpyAsync(ctx->s_gap.p, gap, (size_t)n * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    bool none = false;
    // its own scratch for the bounds, as voxel_downsample: `small` keeps the target's box
    if ((st = voxel_sorted_keys(ctx, "apd_eval_voxel_scores", n, voxel, (uint32_t *)ctx->q_aux.p, none))) return st;
    if (none || num_tol == 0) return deliver();
    const uint64_t *keys = (const uint64_t *)ctx->q_keys_s.p;
    uint64_t *cnt = (uint64_t *)ctx->s_cnt.p;
    unsigned long long *out = (unsigned long long *)ctx->s_out.p;
    HIP_OK(ctx, hipMemsetAsync(out, 0, (size_t)num_tol * 32, s));
    // one tolerance at a time: the scratch is one uint64 per point whatever num_tol is
    for (int k = 0; k < num_tol; ++k) {
        const ClassOf cls{(const int *)ctx->q_idx_s.p, (const float *)ctx->s_dist.p,
                          gap ? (const float *)ctx->s_gap.p : nullptr, tols[(size_t)k]};
        auto vals = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), cls);
        size_t tb = 0;
        HIP_OK(ctx, rocprim::inclusive_scan_by_key(nullptr, tb, keys, vals, cnt, (size_t)n, rocprim::plus<uint64_t>(),
                                                  rocprim::equal_to<uint64_t>(), s));
        if ((st = grow(ctx, ctx->sort_tmp, tb))) return st;
        HIP_OK(ctx, rocprim::inclusive_scan_by_key(ctx->sort_tmp.p, tb, keys, vals, cnt, (size_t)n,
                                                  rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(), s));
        hipLaunchKernelGGL(k_voxel_ratio, dim3(std::min(grid_for(n), RATIO_GRID)), dim3(BLOCK), 0, s, keys,
                           (const uint64_t *)cnt, n,
                           out + 4 * (size_t)k);
        HIP_OK(ctx, hipGetLastError());
    }
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(sums.data(), out, (size_t)num_tol * 32, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if ((st = deliver())) return st;
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->scores_ms);
}

int32_t apd_eval_get_protocol_timing(apd_eval_ctx *ctx, double *free_gap_ms, double *scores_ms) {
    if (!ctx) return APD_EINVAL;
    if (free_gap_ms) *free_gap_ms = ctx->free_gap_ms;
    if (scores_ms) *scores_ms = ctx->scores_ms;
    return APD_OK;
}

// ---- crop volume, nearest neighbour with index, transform, registration ---------------------------

static bool finite16(const double *T) {
    if (!T) return true;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return false;
    return true;
}

static Rows3 rows_of(const double *T) {
    Rows3 M;
    for (int i = 0; i < 12; ++i) M.m[i] = T ? T[i] : (i % 5 == 0 ? 1.0 : 0.0);
    return M;
}

int32_t apd_eval_crop_volume(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const double *T, int32_t axis,
                             double axis_min, double axis_max, int32_t m, const double *poly, int32_t *keep_idx,
                             int64_t *n_keep) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_crop_volume", n64, xyz);
    if (st) return st;
    if (!n_keep || (n64 > 0 && !keep_idx) || !poly) {
        ctx->err = "apd_eval_crop_volume: NULL polygon or output";
        return APD_EINVAL;
    }
    if (m < 3 || m > (1 << 20) || axis < 0 || axis > 2 || !std::isfinite(axis_min) || !std::isfinite(axis_max) ||
        !finite16(T)) {
        ctx->err = "apd_eval_crop_volume: fewer than 3 or more than 2^20 vertices, a bad axis, or a non-finite bound or "
                   "transform";
        return APD_EINVAL;
    }
    for (int i = 0; i < 2 * m; ++i)
        if (!std::isfinite(poly[i])) {
            ctx->err = "apd_eval_crop_volume: a non-finite polygon vertex";
            return APD_EINVAL;
        }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    ctx->crop_ms = 0.0;
    unsigned long long kept = 0;
    if (n == 0) {
        HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
        return APD_OK;
    }
    // q_dist holds the flags, q_aux their exclusive scan from byte 128 and the kept count at byte 64,
    // q_keys the kept indices (the layout of apd_eval_voxel_downsample)
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) || (st = grow(ctx, ctx->q_aux, 128 + (size_t)n * 4)) ||
        (st = grow(ctx, ctx->c_poly, (size_t)m * 16)))
        return st;
    unsigned long long *counter = (unsigned long long *)((char *)ctx->q_aux.p + 64);
    int *flag = (int *)ctx->q_dist.p, *pos = (int *)ctx->q_aux.p + 32, *keep = (int *)ctx->q_keys.p;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->c_poly.p, poly, (size_t)m * 16, hipMemcpyHostToDevice, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(k_crop_flags, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, rows_of(T),
                       T ? 1 : 0, (int)axis, axis_min, axis_max, (int)m, (const double *)ctx->c_poly.p, flag);
    HIP_OK(ctx, hipGetLastError());
    size_t tb = 0;
    HIP_OK(ctx, rocprim::exclusive_scan(nullptr, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    if ((st = grow(ctx, ctx->sort_tmp, tb))) return st;
    HIP_OK(ctx, rocprim::exclusive_scan(ctx->sort_tmp.p, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(k_voxel_compact, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const int *)flag, (const int *)pos, n,
                       keep, counter);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(&kept, counter, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));  // the polygon has been read: the caller's array is free again
    if (kept > 0) HIP_OK(ctx, hipMemcpy(keep_idx, keep, (size_t)kept * 4, hipMemcpyDefault));
    HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->crop_ms);
}

int32_t apd_eval_nearest(apd_eval_ctx *ctx, int64_t n64, const float *xyz, float max_dist, float *dist, int32_t *idx) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_nearest", n64, xyz);
    if (st) return st;
    if (!(max_dist >= 0.0f)) {
        ctx->err = "apd_eval_nearest: max_dist is negative or NaN";
        return APD_EINVAL;
    }
    if (!ctx->has_target) {
        ctx->err = "apd_eval_nearest: no target set";
        return APD_ESTATE;
    }
    const int n = (int)n64;
    ctx->query_ms = 0.0;
    if (n == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->n_idx, (size_t)n * 4)) || (st = grow(ctx, ctx->small, 256)))
        return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    const uint32_t *bounds = (const uint32_t *)ctx->small.p;  // the target's box, as in apd_eval_distances
    hipLaunchKernelGGL(k_morton_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, bounds,
                       (uint64_t *)ctx->q_keys.p, (int *)ctx->q_idx.p, (unsigned long long *)nullptr);
    HIP_OK(ctx, hipGetLastError());
    if ((st = sort_pairs(ctx, ctx->q_keys, ctx->q_keys_s, ctx->q_idx, ctx->q_idx_s, n))) return st;
    hipLaunchKernelGGL(k_nearest_idx, dim3(grid_for(n)), dim3(BLOCK), 0, s, ctx->tree, (const int *)ctx->t_idx_s.p, n,
                       (const uint64_t *)ctx->q_keys_s.p, (const int *)ctx->q_idx_s.p, (const float *)ctx->q_xyz.p,
                       d2_bound(max_dist), max_dist, (float *)ctx->q_dist.p, (int *)ctx->n_idx.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    if (dist) HIP_OK(ctx, hipMemcpyAsync(dist, ctx->q_dist.p, (size_t)n * 4, hipMemcpyDefault, s));
    if (idx) HIP_OK(ctx, hipMemcpyAsync(idx, ctx->n_idx.p, (size_t)n * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->query_ms);
}

int32_t apd_eval_transform(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const double *T, float *out) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_transform", n64, xyz);
    if (st) return st;
    if ((n64 > 0 && !out) || !finite16(T)) {
        ctx->err = "apd_eval_transform: NULL output or a non-finite transform";
        return APD_EINVAL;
    }
    const int n = (int)n64;
    ctx->transform_ms = 0.0;
    if (n == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->x_out, (size_t)n * 12))) return st;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(k_transform, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, rows_of(T),
                       (float *)ctx->x_out.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(out, ctx->x_out.p, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->transform_ms);
}

// uploads the source once; reg_sums then evaluates a transform: the fused kernel, the fold, 19 doubles back
static int reg_upload(apd_eval_ctx *ctx, int n, const float *xyz) {
    int st;
    const int nblocks = (n + APD_REG_BLOCK - 1) / APD_REG_BLOCK;
    if ((st = grow(ctx, ctx->q_xyz, (size_t)std::max(n, 1) * 12)) ||
        (st = grow(ctx, ctx->g_part, (size_t)std::max(nblocks, 1) * APD_REG_SUMS * 8)) ||
        (st = grow(ctx, ctx->g_sums, APD_REG_SUMS * 8)) || (st = grow(ctx, ctx->small, 256)))
        return st;
    if (n > 0) HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, ctx->stream));
    ctx->reg_eval_ms = ctx->reg_fold_ms = ctx->reg_solve_ms = 0.0;
    ctx->reg_evaluations = 0;
    return APD_OK;
}

static int reg_sums(apd_eval_ctx *ctx, int n, const double *T, float max_corr, float bound_d2, double *m) {
    hipStream_t s = ctx->stream;
    const int nblocks = (n + APD_REG_BLOCK - 1) / APD_REG_BLOCK;
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    if (nblocks > 0)
        hipLaunchKernelGGL(k_reg_eval, dim3(nblocks), dim3(BLOCK), 0, s, ctx->tree, (const int *)ctx->t_idx_s.p,
                           (const uint32_t *)ctx->small.p, (const float *)ctx->q_xyz.p, n, rows_of(T), bound_d2, max_corr,
                           (double *)ctx->g_part.p);
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    hipLaunchKernelGGL(k_reg_fold, dim3(1), dim3(64), 0, s, (const double *)ctx->g_part.p, nblocks,
                       (double *)ctx->g_sums.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev2, s));
    HIP_OK(ctx, hipMemcpyAsync(m, ctx->g_sums.p, APD_REG_SUMS * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    float a = 0.0f, b = 0.0f;
    HIP_OK(ctx, hipEventElapsedTime(&a, ctx->ev0, ctx->ev1));
    HIP_OK(ctx, hipEventElapsedTime(&b, ctx->ev1, ctx->ev2));
    ctx->reg_eval_ms += (double)a;
    ctx->reg_fold_ms += (double)b;
    ++ctx->reg_evaluations;
    return APD_OK;
}

static int reg_check(apd_eval_ctx *ctx, const char *what, int64_t n, const float *xyz, const double *T0,
                     float max_corr) {
    int st = check_n(ctx, what, n, xyz);
    if (st) return st;
    if (!finite16(T0) || !(max_corr > 0.0f) || !std::isfinite(max_corr)) {
        ctx->err = std::string(what) + ": a non-finite transform, or max_corr not positive and finite";
        return APD_EINVAL;
    }
    if (!ctx->has_target) {
        ctx->err = std::string(what) + ": no target set";
        return APD_ESTATE;
    }
    return APD_OK;
}

int32_t apd_eval_register_sums(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const double *T, float max_corr,
                               double *sums) {
    if (!ctx) return APD_EINVAL;
    int st = reg_check(ctx, "apd_eval_register_sums", n64, xyz, T, max_corr);
    if (st) return st;
    if (!sums) {
        ctx->err = "apd_eval_register_sums: NULL output";
        return APD_EINVAL;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if ((st = reg_upload(ctx, (int)n64, xyz))) return st;
    return reg_sums(ctx, (int)n64, T, max_corr, d2_bound(max_corr), sums);
}

int32_t apd_eval_register(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const double *T0, float max_corr,
                          int32_t with_scale, int32_t max_iter, double eps_fitness, double eps_rmse, double *T,
                          apd_eval_reg_info *info) {
    if (!ctx) return APD_EINVAL;
    int st = reg_check(ctx, "apd_eval_register", n64, xyz, T0, max_corr);
    if (st) return st;
    if (!T || !info || with_scale < 0 || with_scale > 1 || max_iter < 1 || max_iter > 1000 || !(eps_fitness >= 0.0) ||
        !(eps_rmse >= 0.0)) {
        ctx->err = "apd_eval_register: NULL output, with_scale outside 0..1, max_iter outside 1..1000 or a bad eps";
        return APD_EINVAL;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    if ((st = reg_upload(ctx, n, xyz))) return st;
    const float bound = d2_bound(max_corr);
    // host time of the solves: the loop's wall time minus what it spent waiting on the evaluations
    using clk = std::chrono::steady_clock;
    std::chrono::duration<double, std::milli> waited{0.0};
    const clk::time_point t0 = clk::now();
    st = apd_reg_iterate(T0, with_scale, max_iter, eps_fitness, eps_rmse, T, info, [&](const double *cur, double *m) {
        const clk::time_point a = clk::now();
        const int r = reg_sums(ctx, n, cur, max_corr, bound, m);
        waited += clk::now() - a;
        return (int32_t)r;
    });
    const std::chrono::duration<double, std::milli> total = clk::now() - t0;
    ctx->reg_solve_ms = std::max(0.0, (total - waited).count());
    if (st == APD_ESTATE)
        ctx->err = "apd_eval_register: fewer than 3 correspondences or a degenerate configuration";
    return st;
}

int32_t apd_eval_get_register_timing(apd_eval_ctx *ctx, double *eval_ms, double *fold_ms, double *solve_ms,
                                     int32_t *evaluations, double *crop_ms, double *transform_ms) {
    if (!ctx) return APD_EINVAL;
    if (eval_ms) *eval_ms = ctx->reg_eval_ms;
    if (fold_ms) *fold_ms = ctx->reg_fold_ms;
    if (solve_ms) *solve_ms = ctx->reg_solve_ms;
    if (evaluations) *evaluations = ctx->reg_evaluations;
    if (crop_ms) *crop_ms = ctx->crop_ms;
    if (transform_ms) *transform_ms = ctx->transform_ms;
    return APD_OK;
}

// ---- radius thinning, observability mask, half-space, masked statistics ------------------------------

int32_t apd_eval_radius_thin(apd_eval_ctx *ctx, int64_t n64, const float *xyz, float radius, const uint32_t *rank,
                             int32_t *keep_idx, int64_t *n_keep) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_radius_thin", n64, xyz);
    if (st) return st;
    float r2;
    ThinGrid g{};
    if (!apd_dtu_radius(radius, &r2, &g.cell)) {
        ctx->err = "apd_eval_radius_thin: radius must be positive with a finite, normal fp32 square";
        return APD_EINVAL;
    }
    if (!n_keep || (n64 > 0 && !keep_idx)) {
        ctx->err = "apd_eval_radius_thin: NULL output";
        return APD_EINVAL;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    ctx->thin_sort_ms = ctx->thin_rounds_ms = 0.0;
    ctx->thin_rounds = 0;
    unsigned long long kept = 0;
    if (n == 0) {
        HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
        return APD_OK;
    }
    // q_dist holds the kept flags, q_aux their exclusive scan from byte 128 and the kept count at byte
    // 64, q_keys (free once sorted) the kept indices: the layout of apd_eval_voxel_downsample.
    // th_small: the bounds at byte 0, the finite count at byte 64, the round counters from byte 128.
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) || (st = grow(ctx, ctx->q_idx, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_idx_s, (size_t)n * 4)) || (st = grow(ctx, ctx->q_dist, (size_t)n * 4)) ||
        (st = grow(ctx, ctx->q_aux, 128 + (size_t)n * 4)) || (st = grow(ctx, ctx->th_small, 256)) ||
        (rank && (st = grow(ctx, ctx->th_rank, (size_t)n * 4))))
        return st;
    uint32_t *bounds = (uint32_t *)ctx->th_small.p;
    unsigned long long *n_finite = (unsigned long long *)((char *)ctx->th_small.p + 64);
    unsigned int *cnt = (unsigned int *)((char *)ctx->th_small.p + 128);  // THIN_BATCH + 1 words
    unsigned long long *counter = (unsigned long long *)((char *)ctx->q_aux.p + 64);
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    if (rank) HIP_OK(ctx, hipMemcpyAsync(ctx->th_rank.p, rank, (size_t)n * 4, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    HIP_OK(ctx, hipMemsetAsync(bounds, 0xFF, 12, s));
    HIP_OK(ctx, hipMemsetAsync(bounds + 3, 0, 12, s));
    HIP_OK(ctx, hipMemsetAsync(n_finite, 0, 8, s));
    hipLaunchKernelGGL(k_bounds, dim3(grid_capped(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, bounds);
    HIP_OK(ctx, hipGetLastError());
    uint32_t hb[6];
    HIP_OK(ctx, hipMemcpyAsync(hb, bounds, 24, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if (hb[0] == 0xFFFFFFFFu) {  // no finite point
        HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
        return APD_OK;
    }
    // the cell index is monotone in the coordinate, so the occupied cells span cell(min) .. cell(max)
    for (int a = 0; a < 3; ++a) {
        auto dec = [](uint32_t u) {
            const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
            float f;
            memcpy(&f, &b, 4);
            return f;
        };
        g.lo[a] = apd_dtu_cell(dec(hb[a]), g.cell);
        if (!(apd_dtu_cell(dec(hb[3 + a]), g.cell) - g.lo[a] < APD_DTU_CELL_SPAN)) {
            ctx->err = "apd_eval_radius_thin: an axis spans more than 2^21 cells";
            return APD_EINVAL;
        }
    }
    hipLaunchKernelGGL(k_thin_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, g,
                       (uint64_t *)ctx->q_keys.p, (int *)ctx->q_idx.p, n_finite);
    HIP_OK(ctx, hipGetLastError());
    if ((st = sort_pairs(ctx, ctx->q_keys, ctx->q_keys_s, ctx->q_idx, ctx->q_idx_s, n))) return st;
    unsigned long long nf64 = 0;
    HIP_OK(ctx, hipMemcpyAsync(&nf64, n_finite, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const int nf = (int)nf64;  // >= 1: the bounds saw a finite point
    if ((st = grow(ctx, ctx->th_pts, (size_t)nf * 16)) ||
        (st = grow(ctx, ctx->th_runs, (size_t)nf * THIN_RUNS * sizeof(int2))) ||
        (st = grow(ctx, ctx->th_state, (size_t)nf)) || (st = grow(ctx, ctx->th_list0, (size_t)nf * 4)) ||
        (st = grow(ctx, ctx->th_list1, (size_t)nf * 4)))
        return st;
    const float4 *pts = (const float4 *)ctx->th_pts.p;
    const int *idx_s = (const int *)ctx->q_idx_s.p;
    const int2 *runs = (const int2 *)ctx->th_runs.p;
    uint8_t *state = (uint8_t *)ctx->th_state.p;
    int *lists[2] = {(int *)ctx->th_list0.p, (int *)ctx->th_list1.p};
    hipLaunchKernelGGL(k_thin_gather, dim3(grid_for(nf)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p,
                       rank ? (const uint32_t *)ctx->th_rank.p : (const uint32_t *)nullptr, idx_s, nf,
                       (float4 *)ctx->th_pts.p);
    hipLaunchKernelGGL(k_thin_runs, dim3(grid_for(nf)), dim3(BLOCK), 0, s, (const uint64_t *)ctx->q_keys_s.p, nf,
                       (int2 *)ctx->th_runs.p);
    HIP_OK(ctx, hipMemsetAsync(state, THIN_UNDECIDED, (size_t)nf, s));
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));

    // Rounds until no point is undecided. Round r reads the worklist lists[r & 1] (round 0: every
    // position) and writes lists[(r + 1) & 1]; a batch of rounds shares one read-back of its counters,
    // each round's grid sized by the count at the start of the batch (the counts only fall). Every
    // round decides at least the lowest-key undecided point, so m reaches 0.
    unsigned int m = (unsigned int)nf;
    int round = 0;
    while (m > 0) {
        const int batch = (int)m > THIN_BATCH_BELOW ? 1 : THIN_BATCH;
        HIP_OK(ctx, hipMemsetD32Async((hipDeviceptr_t)cnt, (int)m, 1, s));
        HIP_OK(ctx, hipMemsetAsync(cnt + 1, 0, (size_t)batch * 4, s));
        for (int k = 0; k < batch; ++k, ++round)
            hipLaunchKernelGGL(k_thin_round, dim3(grid_for(m)), dim3(BLOCK), 0, s, pts, idx_s, runs, nf, r2,
                               round == 0 ? (const int *)nullptr : (const int *)lists[round & 1],
                               (const unsigned int *)(cnt + k), state, lists[(round + 1) & 1], cnt + k + 1);
        HIP_OK(ctx, hipGetLastError());
        unsigned int hc[THIN_BATCH];
        HIP_OK(ctx, hipMemcpyAsync(hc, cnt + 1, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        int used = batch;  // the rounds of this batch up to the first that left nothing
        for (int k = 0; k < batch; ++k)
            if (hc[k] == 0) {
                used = k + 1;
                break;
            }
        ctx->thin_rounds += used;
        if (hc[batch - 1] >= m) {  // cannot happen: a round decides at least one point
            ctx->err = "apd_eval_radius_thin: a round decided nothing";
            return APD_EDEVICE;
        }
        m = hc[batch - 1];
    }

    int *flag = (int *)ctx->q_dist.p, *pos = (int *)ctx->q_aux.p + 32, *keep = (int *)ctx->q_keys.p;
    HIP_OK(ctx, hipMemsetAsync(flag, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(k_thin_flags, dim3(grid_for(nf)), dim3(BLOCK), 0, s, (const uint8_t *)state, idx_s, nf, flag);
    HIP_OK(ctx, hipGetLastError());
    size_t tb = 0;
    HIP_OK(ctx, rocprim::exclusive_scan(nullptr, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    if ((st = grow(ctx, ctx->sort_tmp, tb))) return st;
    HIP_OK(ctx, rocprim::exclusive_scan(ctx->sort_tmp.p, tb, flag, pos, 0, (size_t)n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(k_voxel_compact, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const int *)flag, (const int *)pos, n,
                       keep, counter);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev2, s));
    HIP_OK(ctx, hipMemcpyAsync(&kept, counter, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if (kept > 0) HIP_OK(ctx, hipMemcpy(keep_idx, keep, (size_t)kept * 4, hipMemcpyDefault));
    HIP_OK(ctx, hipMemcpy(n_keep, &kept, 8, hipMemcpyDefault));
    if ((st = event_ms(ctx, ctx->ev0, ctx->ev1, ctx->thin_sort_ms))) return st;
    return event_ms(ctx, ctx->ev1, ctx->ev2, ctx->thin_rounds_ms);
}

int32_t apd_eval_get_thin_timing(apd_eval_ctx *ctx, double *sort_ms, double *rounds_ms, int32_t *rounds) {
    if (!ctx) return APD_EINVAL;
    if (sort_ms) *sort_ms = ctx->thin_sort_ms;
    if (rounds_ms) *rounds_ms = ctx->thin_rounds_ms;
    if (rounds) *rounds = ctx->thin_rounds;
    return APD_OK;
}

int32_t apd_eval_obs_mask(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const int32_t dims[3],
                          const double origin[3], double res, const uint8_t *mask, uint8_t *inside) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_obs_mask", n64, xyz);
    if (st) return st;
    if (!dims || !origin || !mask || (n64 > 0 && !inside)) {
        ctx->err = "apd_eval_obs_mask: NULL dims, origin, mask or output";
        return APD_EINVAL;
    }
    apd_dtu_mask_geom g;
    double total = 1.0;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 1 || !std::isfinite(origin[k])) {
            ctx->err = "apd_eval_obs_mask: a dim below 1 or a non-finite origin";
            return APD_EINVAL;
        }
        g.dims[k] = dims[k];
        g.origin[k] = origin[k];
        total *= (double)dims[k];
    }
    if (total > 2147483648.0) {
        ctx->err = "apd_eval_obs_mask: the mask has more than 2^31 cells";
        return APD_EINVAL;
    }
    if (!(res > 0.0) || !std::isfinite(res)) {
        ctx->err = "apd_eval_obs_mask: res must be positive and finite";
        return APD_EINVAL;
    }
    g.res = res;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int n = (int)n64;
    ctx->mask_ms = 0.0;
    hipStream_t s = ctx->stream;
    if (ctx->mask_src != mask || memcmp(ctx->mask_dims, dims, 12) != 0) {
        ctx->mask_src = nullptr;
        if ((st = grow(ctx, ctx->m_mask, (size_t)total))) return st;
        HIP_OK(ctx, hipMemcpyAsync(ctx->m_mask.p, mask, (size_t)total, hipMemcpyDefault, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        ctx->mask_src = mask;
        memcpy(ctx->mask_dims, dims, 12);
    }
    if (n == 0) return APD_OK;
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->d_flag, (size_t)n))) return st;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(k_obs_mask, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, g,
                       (const uint8_t *)ctx->m_mask.p, (uint8_t *)ctx->d_flag.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(inside, ctx->d_flag.p, (size_t)n, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->mask_ms);
}

int32_t apd_eval_half_space(apd_eval_ctx *ctx, int64_t n64, const float *xyz, const double P[4], uint8_t *above) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_half_space", n64, xyz);
    if (st) return st;
    if (!P || (n64 > 0 && !above)) {
        ctx->err = "apd_eval_half_space: NULL plane or output";
        return APD_EINVAL;
    }
    const int n = (int)n64;
    ctx->half_space_ms = 0.0;
    if (n == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if ((st = grow(ctx, ctx->q_xyz, (size_t)n * 12)) || (st = grow(ctx, ctx->d_flag, (size_t)n))) return st;
    Plane4 pl;
    for (int k = 0; k < 4; ++k) pl.P[k] = P[k];
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->q_xyz.p, xyz, (size_t)n * 12, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    hipLaunchKernelGGL(k_half_space, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const float *)ctx->q_xyz.p, n, pl,
                       (uint8_t *)ctx->d_flag.p);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    HIP_OK(ctx, hipMemcpyAsync(above, ctx->d_flag.p, (size_t)n, hipMemcpyDefault, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->half_space_ms);
}

int32_t apd_eval_masked_stats(apd_eval_ctx *ctx, int64_t n64, const float *dist, const uint8_t *flag, float limit,
                              int64_t *count, double *sum, double *median) {
    if (!ctx) return APD_EINVAL;
    int st = check_n(ctx, "apd_eval_masked_stats", n64, dist);
    if (st) return st;
    if (limit != limit) {
        ctx->err = "apd_eval_masked_stats: the limit is NaN";
        return APD_EINVAL;
    }
    const int n = (int)n64;
    ctx->stats_ms = 0.0;
    if (count) *count = 0;
    if (sum) *sum = 0.0;
    if (median) *median = 0.0;
    if (n == 0) return APD_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const int nblocks = (int)((n64 + APD_REG_BLOCK - 1) / APD_REG_BLOCK);
    // s_dist: the distances; q_keys / q_keys_s: the 32-bit sort keys and their sorted copy;
    // st_out: the sum at byte 0, the count at byte 8
    if ((st = grow(ctx, ctx->s_dist, (size_t)n * 4)) || (flag && (st = grow(ctx, ctx->d_flag, (size_t)n))) ||
        (st = grow(ctx, ctx->q_keys, (size_t)n * 8)) || (st = grow(ctx, ctx->q_keys_s, (size_t)n * 8)) ||
        (st = grow(ctx, ctx->st_part, (size_t)nblocks * 8)) || (st = grow(ctx, ctx->st_out, 64)))
        return st;
    uint32_t *keys = (uint32_t *)ctx->q_keys.p, *keys_s = (uint32_t *)ctx->q_keys_s.p;
    double *out = (double *)ctx->st_out.p;
    unsigned long long *cnt = (unsigned long long *)ctx->st_out.p + 1;
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(ctx->s_dist.p, dist, (size_t)n * 4, hipMemcpyDefault, s));
    if (flag) HIP_OK(ctx, hipMemcpyAsync(ctx->d_flag.p, flag, (size_t)n, hipMemcpyDefault, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev0, s));
    HIP_OK(ctx, hipMemsetAsync(cnt, 0, 8, s));
    hipLaunchKernelGGL(k_stats_block, dim3(nblocks), dim3(BLOCK), 0, s, (const float *)ctx->s_dist.p,
                       flag ? (const uint8_t *)ctx->d_flag.p : (const uint8_t *)nullptr, n, limit,
                       (double *)ctx->st_part.p, keys, cnt);
    hipLaunchKernelGGL(k_stats_fold, dim3(1), dim3(64), 0, s, (const double *)ctx->st_part.p, nblocks, out);
    HIP_OK(ctx, hipGetLastError());
    size_t tb = 0;
    HIP_OK(ctx, rocprim::radix_sort_keys(nullptr, tb, keys, keys_s, (size_t)n, 0, 32, s));
    if ((st = grow(ctx, ctx->sort_tmp, tb))) return st;
    HIP_OK(ctx, rocprim::radix_sort_keys(ctx->sort_tmp.p, tb, keys, keys_s, (size_t)n, 0, 32, s));
    HIP_OK(ctx, hipEventRecord(ctx->ev1, s));
    struct {
        double sum;
        unsigned long long count;
    } h{};
    HIP_OK(ctx, hipMemcpyAsync(&h, ctx->st_out.p, 16, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    double med = 0.0;
    if (h.count > 0) {
        const size_t m = (size_t)h.count, a = (m - 1) / 2, b = m / 2;  // a == b for an odd count
        uint32_t mid[2];
        HIP_OK(ctx, hipMemcpy(&mid[0], keys_s + a, 4, hipMemcpyDeviceToHost));
        HIP_OK(ctx, hipMemcpy(&mid[1], keys_s + b, 4, hipMemcpyDeviceToHost));
        float v[2];
        for (int k = 0; k < 2; ++k) {
            const uint32_t u = (mid[k] & 0x80000000u) ? (mid[k] & 0x7FFFFFFFu) : ~mid[k];
            memcpy(&v[k], &u, 4);
        }
        med = a == b ? (double)v[0] : ((double)v[0] + (double)v[1]) / 2.0;
    }
    if (count) *count = (int64_t)h.count;
    if (sum) *sum = h.sum;
    if (median) *median = med;
    return event_ms(ctx, ctx->ev0, ctx->ev1, ctx->stats_ms);
}

int32_t apd_eval_get_dtu_timing(apd_eval_ctx *ctx, double *mask_ms, double *half_space_ms, double *stats_ms) {
    if (!ctx) return APD_EINVAL;
    if (mask_ms) *mask_ms = ctx->mask_ms;
    if (half_space_ms) *half_space_ms = ctx->half_space_ms;
    if (stats_ms) *stats_ms = ctx->stats_ms;
    return APD_OK;
}

}  // extern "C"
