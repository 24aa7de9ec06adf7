// apd_seg_host.cpp — the host-only entries of include/apd_seg.h: the five stages on the CPU, one
// thread, whole-image loops and a breadth-first labelling (the device path's baseline and what the
// CPU tests run). No HIP call: it is part of libapd_hip.so and also builds alone (host/Makefile,
// sanitize-segment).
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/apd_seg.h"
#include "apd_seg.h"

namespace {

using namespace apd_sg;

// Stage 4: a raster scan meets a component first at its smallest index, which is its root; the
// component is then flooded from there. roots = -1 where the mask is 0.
void label_bfs(int W, int H, const uint8_t *mask, int32_t *roots) {
    const int64_t N = (int64_t)W * H;
    for (int64_t i = 0; i < N; ++i) roots[i] = -1;
    std::vector<int32_t> queue;
    for (int64_t i = 0; i < N; ++i) {
        if (!mask[i] || roots[i] >= 0) continue;
        const int32_t root = (int32_t)i;
        roots[i] = root;
        queue.clear();
        queue.push_back(root);
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t p = queue[head];
            const int x = p % W, y = p / W;
            const int32_t nb[4] = {x > 0 ? p - 1 : -1, x + 1 < W ? p + 1 : -1, y > 0 ? p - W : -1,
                                   y + 1 < H ? p + W : -1};
            for (int32_t q : nb)
                if (q >= 0 && mask[q] && roots[q] < 0) {
                    roots[q] = root;
                    queue.push_back(q);
                }
        }
    }
}

}  // namespace

extern "C" {

int32_t apd_seg_working_size(int32_t w, int32_t h, int32_t max_size, int32_t *s, int32_t *W, int32_t *H) {
    if (w < 1 || w > APD_SEG_MAX_SIDE || h < 1 || h > APD_SEG_MAX_SIDE || max_size < 0) return APD_EINVAL;
    const int f = scale_of(w, h, max_size);
    if (check_size(ceil_div(w, f), ceil_div(h, f))) return APD_EINVAL;
    if (s) *s = f;
    if (W) *W = ceil_div(w, f);
    if (H) *H = ceil_div(h, f);
    return APD_OK;
}

void apd_seg_label_colour(int32_t k, uint8_t bgr[3]) {
    if (k <= 0 || k > APD_SEG_MAX_LABELS) {
        bgr[0] = bgr[1] = bgr[2] = 255;
        return;
    }
    bgr[0] = (uint8_t)((37 * k + 11) % 224);
    bgr[1] = (uint8_t)((91 * k + 53) % 224);
    bgr[2] = (uint8_t)((151 * k + 101) % 224);
}

int32_t apd_seg_label_mask_host(int32_t W, int32_t H, const uint8_t *mask_u8, int32_t *roots_i32) {
    if (check_label_mask(W, H, mask_u8, roots_i32)) return APD_EINVAL;
    try {
        label_bfs(W, H, mask_u8, roots_i32);
    } catch (const std::bad_alloc &) {
        return APD_ENOMEM;
    }
    return APD_OK;
}

int32_t apd_seg_flat_zones_bgr8_host(int32_t w, int32_t h, const uint8_t *src, int32_t max_size, int32_t threshold_q8,
                                     int32_t min_area, uint8_t *labels, int32_t *out_w, int32_t *out_h,
                                     int32_t *n_survivors, int32_t *n_labels, uint8_t *work_out, uint16_t *smooth_out,
                                     uint8_t *flat_out, int32_t *roots_out, int32_t *areas_out) {
    if (check_flat_zones(w, h, src, max_size, threshold_q8, min_area, labels, out_w, out_h)) return APD_EINVAL;
    const int s = scale_of(w, h, max_size);
    const int W = ceil_div(w, s), H = ceil_div(h, s);
    const size_t N = (size_t)W * (size_t)H;
    try {
        // 1. downscale
        std::vector<uint8_t> work_own;
        const uint8_t *work = src;
        if (s > 1) {
            work_own.resize(3 * N);
            for (int Y = 0; Y < H; ++Y)
                for (int X = 0; X < W; ++X)
                    for (int c = 0; c < 3; ++c) work_own[((size_t)Y * W + X) * 3 + c] = box_mean(src, w, h, s, X, Y, c);
            work = work_own.data();
        }
        // 2. smooth: T (horizontal), then S (vertical), planar
        std::vector<uint16_t> T(3 * N), S(3 * N);
        for (int c = 0; c < 3; ++c) {
            uint16_t *t = T.data() + (size_t)c * N;
            for (int y = 0; y < H; ++y) {
                const uint8_t *row = work + (size_t)y * W * 3 + c;
                for (int x = 0; x < W; ++x) {
                    auto at = [&](int d) { return (int)row[(size_t)clampi(x + d, 0, W - 1) * 3]; };
                    t[(size_t)y * W + x] = (uint16_t)tap5(at(-2), at(-1), at(0), at(1), at(2));
                }
            }
            uint16_t *sp = S.data() + (size_t)c * N;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    auto at = [&](int d) { return (int)t[(size_t)clampi(y + d, 0, H - 1) * W + x]; };
                    sp[(size_t)y * W + x] = (uint16_t)tap5(at(-2), at(-1), at(0), at(1), at(2));
                }
        }
        T = std::vector<uint16_t>();
        // 3. flatness
        std::vector<uint8_t> flat(N);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int g = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        for (int c = 0; c < 3; ++c) {
                            const int d = absdiff(S[(size_t)c * N + (size_t)y * W + x], S[(size_t)c * N + (size_t)qy * W + qx]);
                            if (d > g) g = d;
                        }
                    }
                flat[(size_t)y * W + x] = g <= threshold_q8 ? 1 : 0;
            }
        // 4. components
        std::vector<int32_t> roots(N);
        label_bfs(W, H, flat.data(), roots.data());
        // 5. areas and ranking
        std::vector<int32_t> areas(N, 0);
        for (size_t i = 0; i < N; ++i)
            if (roots[i] >= 0) ++areas[(size_t)roots[i]];
        std::vector<uint64_t> keys;
        for (size_t i = 0; i < N; ++i)
            if (areas[i] >= min_area) keys.push_back(rank_key(areas[i], (int32_t)i));
        const size_t top = std::min<size_t>(keys.size(), APD_SEG_MAX_LABELS);
        std::partial_sort(keys.begin(), keys.begin() + (ptrdiff_t)top, keys.end());
        LabelTable table;
        table_from_ranked(keys.data(), (int)top, table);
        for (size_t i = 0; i < N; ++i)
            labels[i] = roots[i] >= 0 ? label_of(table.root, table.label, table.n, roots[i]) : (uint8_t)0;
        *out_w = W;
        *out_h = H;
        if (n_survivors) *n_survivors = (int32_t)keys.size();
        if (n_labels) *n_labels = (int32_t)top;
        if (work_out) std::memcpy(work_out, work, 3 * N);
        if (smooth_out) std::memcpy(smooth_out, S.data(), 3 * N * sizeof(uint16_t));
        if (flat_out) std::memcpy(flat_out, flat.data(), N);
        if (roots_out) std::memcpy(roots_out, roots.data(), N * sizeof(int32_t));
        if (areas_out) std::memcpy(areas_out, areas.data(), N * sizeof(int32_t));
    } catch (const std::bad_alloc &) {
        return APD_ENOMEM;
    }
    return APD_OK;
}

}  // extern "C"
