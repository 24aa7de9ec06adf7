// apd_seg.h — the arithmetic of include/apd_seg.h's contract that the host (apd_seg_host.cpp) and the
// device (apd_seg.hip) share: the working size, the rounded box mean, the binomial taps, the channel
// distance, the argument rules and the ranking of the survivors. Integers only.
#ifndef APD_SEG_SHARED_H_
#define APD_SEG_SHARED_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/apd_seg.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APD_SEG_HD __host__ __device__ __forceinline__
#else
#define APD_SEG_HD inline
#endif

namespace apd_sg {

// stage 1: the factor and the working size
APD_SEG_HD int scale_of(int w, int h, int max_size) {
    const int m = w > h ? w : h;
    return (max_size == 0 || m <= max_size) ? 1 : (m + max_size - 1) / max_size;
}
APD_SEG_HD int ceil_div(int a, int b) { return (a + b - 1) / b; }

// stage 1: one channel of one working pixel; src is interleaved BGR of w x h
APD_SEG_HD uint8_t box_mean(const uint8_t *src, int w, int h, int s, int X, int Y, int c) {
    const int x0 = X * s, y0 = Y * s;
    const int x1 = (w - x0 < s) ? w : x0 + s, y1 = (h - y0 < s) ? h : y0 + s;
    uint64_t sum = 0;
    for (int y = y0; y < y1; ++y) {
        const uint8_t *row = src + ((size_t)y * (size_t)w + (size_t)x0) * 3 + c;
        for (int x = x0; x < x1; ++x, row += 3) sum += *row;
    }
    const uint64_t cnt = (uint64_t)(x1 - x0) * (uint64_t)(y1 - y0);
    return (uint8_t)((2 * sum + cnt) / (2 * cnt));
}

// stage 2: five taps of the binomial filter, not normalised
APD_SEG_HD int tap5(int a, int b, int c, int d, int e) { return a + 4 * b + 6 * c + 4 * d + e; }

APD_SEG_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// stage 3: |a - b| of two S values
APD_SEG_HD int absdiff(int a, int b) { return a > b ? a - b : b - a; }

// The argument rules, one text for the host and the device entries: nullptr or what is wrong.
inline const char *check_size(int W, int H) {
    if (W < 1 || W > APD_SEG_MAX_SIDE || H < 1 || H > APD_SEG_MAX_SIDE) return "a size outside 1..65536";
    if ((int64_t)W * (int64_t)H > (int64_t)INT32_MAX) return "more than INT32_MAX pixels";
    return nullptr;
}
inline const char *check_flat_zones(int w, int h, const void *src, int max_size, int threshold_q8, int min_area,
                                    const void *labels, const void *out_w, const void *out_h) {
    if (w < 1 || w > APD_SEG_MAX_SIDE || h < 1 || h > APD_SEG_MAX_SIDE) return "a size outside 1..65536";
    if (max_size < 0) return "a negative max_size";
    if (threshold_q8 < 0 || threshold_q8 > APD_SEG_MAX_THRESHOLD_Q8) return "threshold_q8 outside 0..65280";
    if (min_area < 1) return "min_area below 1";
    if (!src || !labels || !out_w || !out_h) return "a NULL pointer";
    const int s = scale_of(w, h, max_size);
    return check_size(ceil_div(w, s), ceil_div(h, s));
}
inline const char *check_label_mask(int W, int H, const void *mask, const void *roots) {
    if (const char *what = check_size(W, H)) return what;
    return (!mask || !roots) ? "a NULL pointer" : nullptr;
}

// Stage 5 on the host, for both paths: survivors as keys (0xFFFFFFFF - area) << 32 | root, so that
// ascending keys are area descending, root ascending. The first min(n, 255) keys in that order ->
// their roots ascending with the label of each (the relabelling searches this table).
inline uint64_t rank_key(int32_t area, int32_t root) {
    return ((uint64_t)(0xFFFFFFFFu - (uint32_t)area) << 32) | (uint32_t)root;
}
struct LabelTable {
    int n = 0;
    int32_t root[APD_SEG_MAX_LABELS];
    uint8_t label[APD_SEG_MAX_LABELS];
};
inline void table_from_ranked(const uint64_t *keys, int n, LabelTable &t) {
    std::vector<std::pair<int32_t, uint8_t>> v;
    for (int k = 0; k < n && k < APD_SEG_MAX_LABELS; ++k)
        v.push_back({(int32_t)(uint32_t)(keys[k] & 0xFFFFFFFFu), (uint8_t)(k + 1)});
    std::sort(v.begin(), v.end());
    t.n = (int)v.size();
    for (int k = 0; k < t.n; ++k) {
        t.root[k] = v[(size_t)k].first;
        t.label[k] = v[(size_t)k].second;
    }
}
// the label of a root (0 if it is not in the table): a binary search over at most 255 entries
APD_SEG_HD uint8_t label_of(const int32_t *root, const uint8_t *label, int n, int32_t r) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (root[mid] < r) lo = mid + 1; else hi = mid;
    }
    return (lo < n && root[lo] == r) ? label[lo] : (uint8_t)0;
}

}  // namespace apd_sg

#endif  // APD_SEG_SHARED_H_
