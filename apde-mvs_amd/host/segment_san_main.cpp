// segment_san_main.cpp — the host-only entries of include/apd_seg.h (csrc/apd_seg_host.cpp) as a
// stand-alone program for AddressSanitizer + UBSan (make sanitize-segment): apd_seg_label_mask_host over
// small masks (1 x 1, 1 x 97, 97 x 1, empty, full, checkerboard, serpentine, comb, random), the five
// stages over small images with every stage asked for and with none, rejected arguments, and a few
// truncated or garbled sa_masks bin-mats through the reader (io.cpp). The buffers are heap blocks of
// the exact size, so a read or write past either end is reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/apd_seg.h"
#include "io.h"

namespace {

uint32_t g_state = 2463534242u;
uint32_t next_u32() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

int g_fail = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++g_fail;
    }
}

enum Shape { ZEROS, ONES, CHECKER, SERPENTINE, COMB, RANDOM };

long label(int W, int H, Shape shape) {
    const size_t N = (size_t)W * H;
    uint8_t *mask = (uint8_t *)std::malloc(N);
    int32_t *roots = (int32_t *)std::malloc(N * sizeof(int32_t));
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint8_t v = 0;
            switch (shape) {
                case ZEROS: v = 0; break;
                case ONES: v = 255; break;
                case CHECKER: v = (uint8_t)((x + y) % 2 == 0); break;
                case SERPENTINE: v = (uint8_t)(y % 2 == 0 || x == ((y / 2) % 2 == 0 ? W - 1 : 0)); break;
                case COMB: v = (uint8_t)(y == H - 1 || x % 2 == 0); break;
                default: v = (uint8_t)(next_u32() % 100 < 59); break;
            }
            mask[(size_t)y * W + x] = v;
        }
    expect(apd_seg_label_mask_host(W, H, mask, roots) == APD_OK, "apd_seg_label_mask_host");
    long comps = 0;
    for (size_t i = 0; i < N; ++i) {
        expect((roots[i] >= 0) == (mask[i] != 0) && roots[i] <= (int32_t)i, "a root is -1 off the mask, else at most the index");
        comps += roots[i] == (int32_t)i;
    }
    std::free(mask);
    std::free(roots);
    return comps;
}

void zones(int w, int h, int max_size, int thr, int min_area, bool stages, int kind) {
    uint8_t *src = (uint8_t *)std::malloc(3 * (size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                const int base = kind == 0 ? 128 : kind == 1 ? 40 + 150 * (((x / 9) + (y / 7)) % 2) : (int)(next_u32() % 256);
                src[((size_t)y * w + x) * 3 + c] = (uint8_t)(base + (kind == 1 ? (int)(next_u32() % 3) : 0));
            }
    int32_t s = 0, W = 0, H = 0;
    expect(apd_seg_working_size(w, h, max_size, &s, &W, &H) == APD_OK, "apd_seg_working_size");
    const size_t N = (size_t)W * H;
    uint8_t *labels = (uint8_t *)std::malloc(N);
    uint8_t *work = stages ? (uint8_t *)std::malloc(3 * N) : nullptr;
    uint16_t *smooth = stages ? (uint16_t *)std::malloc(6 * N) : nullptr;
    uint8_t *flat = stages ? (uint8_t *)std::malloc(N) : nullptr;
    int32_t *roots = stages ? (int32_t *)std::malloc(4 * N) : nullptr;
    int32_t *areas = stages ? (int32_t *)std::malloc(4 * N) : nullptr;
    int32_t ow = 0, oh = 0, ns = -1, nl = -1;
    expect(apd_seg_flat_zones_bgr8_host(w, h, src, max_size, thr, min_area, labels, &ow, &oh, &ns, &nl, work, smooth, flat,
                                        roots, areas) == APD_OK, "apd_seg_flat_zones_bgr8_host");
    expect(ow == W && oh == H && ns >= nl && nl >= 0 && nl <= APD_SEG_MAX_LABELS, "sizes and counts");
    int top = 0;
    for (size_t i = 0; i < N; ++i) top = labels[i] > top ? labels[i] : top;
    expect(top == nl, "the largest label is n_labels");
    if (kind == 0) expect(ns == ((int64_t)N >= min_area ? 1 : 0), "a constant image is one region");
    std::free(src);
    std::free(labels);
    std::free(work);
    std::free(smooth);
    std::free(flat);
    std::free(roots);
    std::free(areas);
}

void write_file(const std::string &path, const void *p, size_t n) {
    std::ofstream o(path, std::ios::binary);
    o.write((const char *)p, (std::streamsize)n);
}

}  // namespace

int main() {
    long calls = 0;
    const int sizes[][2] = {{1, 1}, {1, 97}, {97, 1}, {2, 2}, {5, 3}, {64, 16}, {65, 17}, {70, 50}};
    for (const auto &sz : sizes)
        for (int shape = ZEROS; shape <= RANDOM; ++shape) {
            const long comps = label(sz[0], sz[1], (Shape)shape);
            if (shape == ZEROS) expect(comps == 0, "no component in an empty mask");
            if (shape == ONES || shape == SERPENTINE || shape == COMB) expect(comps == 1, "one component");
            if (shape == CHECKER) expect(comps == ((long)sz[0] * sz[1] + 1) / 2, "every set pixel of a checkerboard is its own component");
            ++calls;
        }
    for (const auto &sz : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            zones(sz[0], sz[1], 0, 256, 1, true, kind);
            zones(sz[0], sz[1], 0, 0, 4, false, kind);
            zones(sz[0], sz[1], 2, 256, 1, true, kind);      // s up to 49, partial blocks
            zones(sz[0], sz[1], 23, 65280, 3, false, kind);  // everything flat
            calls += 4;
        }

    // rejected arguments: nothing is read or written
    uint8_t px[12] = {0};
    uint8_t lab[4];
    int32_t ow, oh, roots[4];
    auto fz = [&](int w, int h, const uint8_t *src, int max_size, int thr, int min_area, uint8_t *l, int32_t *pw, int32_t *ph) {
        return apd_seg_flat_zones_bgr8_host(w, h, src, max_size, thr, min_area, l, pw, ph, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr);
    };
    expect(fz(2, 2, px, 0, 256, 1, lab, &ow, &oh) == APD_OK, "the accepted call");
    expect(fz(0, 2, px, 0, 256, 1, lab, &ow, &oh) == APD_EINVAL && fz(2, 65537, px, 0, 256, 1, lab, &ow, &oh) == APD_EINVAL, "size");
    expect(fz(65536, 65536, px, 0, 256, 1, lab, &ow, &oh) == APD_EINVAL, "more than INT32_MAX working pixels");
    expect(fz(2, 2, px, -1, 256, 1, lab, &ow, &oh) == APD_EINVAL, "max_size");
    expect(fz(2, 2, px, 0, -1, 1, lab, &ow, &oh) == APD_EINVAL && fz(2, 2, px, 0, 65281, 1, lab, &ow, &oh) == APD_EINVAL, "threshold");
    expect(fz(2, 2, px, 0, 256, 0, lab, &ow, &oh) == APD_EINVAL, "min_area");
    expect(fz(2, 2, nullptr, 0, 256, 1, lab, &ow, &oh) == APD_EINVAL && fz(2, 2, px, 0, 256, 1, nullptr, &ow, &oh) == APD_EINVAL &&
               fz(2, 2, px, 0, 256, 1, lab, nullptr, &oh) == APD_EINVAL && fz(2, 2, px, 0, 256, 1, lab, &ow, nullptr) == APD_EINVAL,
           "NULL");
    expect(apd_seg_label_mask_host(0, 1, px, roots) == APD_EINVAL && apd_seg_label_mask_host(1, 65537, px, roots) == APD_EINVAL &&
               apd_seg_label_mask_host(65536, 65536, px, roots) == APD_EINVAL && apd_seg_label_mask_host(2, 2, nullptr, roots) == APD_EINVAL &&
               apd_seg_label_mask_host(2, 2, px, nullptr) == APD_EINVAL, "label_mask arguments");
    expect(apd_seg_working_size(0, 1, 0, nullptr, nullptr, nullptr) == APD_EINVAL && apd_seg_working_size(4, 4, -1, nullptr, nullptr, nullptr) == APD_EINVAL &&
               apd_seg_working_size(5, 3, 2, nullptr, nullptr, nullptr) == APD_OK, "working_size arguments");
    uint8_t bgr[3];
    for (int k = -1; k <= 256; ++k) {
        apd_seg_label_colour(k, bgr);
        expect((k >= 1 && k <= 255) ? (bgr[0] < 224 && bgr[1] < 224 && bgr[2] < 224) : (bgr[0] == 255 && bgr[1] == 255 && bgr[2] == 255), "colour");
    }

    // sa_masks bin-mats through the reader: whole, cut anywhere, and with a lying header
    const char *tmp = std::getenv("TMPDIR");
    const std::string path = std::string(tmp && *tmp ? tmp : "/tmp") + "/apd_segment_san_mask.bin";
    std::vector<uint8_t> file(16 + 7 * 5);
    const int32_t hdr[4] = {1, 5, 7, apdhost::CV_8UC1};
    std::memcpy(file.data(), hdr, 16);
    for (size_t i = 16; i < file.size(); ++i) file[i] = (uint8_t)(i % 4);
    apdhost::Mat m;
    write_file(path, file.data(), file.size());
    expect(apdhost::read_binmat_file(path, m) && m.rows == 5 && m.cols == 7 && m.type == apdhost::CV_8UC1 && m.ptr<uint8_t>()[34] == (16 + 34) % 4,
           "a whole mask");
    for (size_t cut : {(size_t)0, (size_t)3, (size_t)15, (size_t)16, (size_t)17, file.size() - 1}) {
        write_file(path, file.data(), cut);
        apdhost::Mat t;
        expect(!apdhost::read_binmat_file(path, t) && t.empty(), "a truncated mask is refused");
    }
    const int32_t lies[][4] = {{2, 5, 7, 0}, {1, -5, 7, 0}, {1, 5, 7, 99}, {1, 1 << 30, 1 << 30, 0}, {1, 5, 8, 0}};
    for (const auto &l : lies) {
        std::memcpy(file.data(), l, 16);
        write_file(path, file.data(), file.size());
        apdhost::Mat t;
        expect(!apdhost::read_binmat_file(path, t), "a lying header is refused");
    }
    std::remove(path.c_str());
    std::printf("segment sanitizer run: %ld calls, %d failures\n", calls, g_fail);
    return g_fail ? 1 : 0;
}
