// undistort_san_main.cpp — the host-only undistortion entries (csrc/apd_undistort_host.cpp) as a
// stand-alone program for AddressSanitizer + UBSan (make sanitize-undistort): every model on a 64x48
// image with corners outside the source, another output size, 1x1 and 3x2 sources, parameters that
// drive the source coordinates to +-1e300 and NaN, rejected arguments, and the keypoint inverse.
// The buffers are heap blocks of the exact size, so a read or write past either end is reported.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/apd_prep.h"

namespace {

uint32_t g_state = 12345u;
uint32_t next_u32() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

struct Model {
    int id, n;
    double p[12];
};

int g_fail = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++g_fail;
    }
}

// the warp into exact-size heap blocks; returns the number of non-black bytes
long warp(const Model &m, int sw, int sh, const double *K, int ow, int oh, int want = APD_OK) {
    uint8_t *src = (uint8_t *)std::malloc(3 * (size_t)sw * sh);
    uint8_t *dst = (uint8_t *)std::malloc(3 * (size_t)ow * oh);
    for (size_t i = 0; i < 3 * (size_t)sw * sh; ++i) src[i] = (uint8_t)(1 + next_u32() % 255);
    std::memset(dst, 7, 3 * (size_t)ow * oh);
    const int st = apd_prep_undistort_bgr8_host(m.id, m.p, m.n, sw, sh, src, K, ow, oh, dst);
    expect(st == want, "status of apd_prep_undistort_bgr8_host");
    long lit = 0;
    for (size_t i = 0; i < 3 * (size_t)ow * oh; ++i) lit += dst[i] != 0;
    std::free(src);
    std::free(dst);
    return lit;
}

}  // namespace

int main() {
    const Model models[] = {
        {0, 3, {50, 30.5, 22.25}},
        {1, 4, {50, 51, 30.5, 22.25}},
        {2, 4, {50, 30.5, 22.25, -0.12}},
        {3, 5, {50, 30.5, 22.25, 0.1, -0.03}},
        {4, 8, {50, 51, 30.5, 22.25, -0.15, 0.05, 0.004, -0.003}},
        {5, 8, {50, 51, 30.5, 22.25, 0.05, -0.02, 0.004, -0.001}},
        {6, 12, {50, 51, 30.5, 22.25, -0.15, 0.05, 0.004, -0.003, 0.01, 0.02, -0.01, 0.003}},
        {8, 4, {50, 30.5, 22.25, 0.03}},
        {9, 5, {50, 30.5, 22.25, 0.03, -0.01}},
        {10, 12, {50, 51, 30.5, 22.25, 0.05, -0.02, 0.004, -0.003, 0.004, -0.001, 0.002, -0.002}},
    };
    long calls = 0;
    for (const Model &m : models) {
        const bool one_f = m.n == 3 || (m.n <= 5 && m.id != 1);
        const double K[4] = {m.p[0], one_f ? m.p[0] : m.p[1], m.p[one_f ? 1 : 2], m.p[one_f ? 2 : 3]};
        expect(warp(m, 64, 48, K, 64, 48) > 0, "64x48");
        const double wide[4] = {20, 20, 30.5, 22.25};  // corners far outside the source
        warp(m, 64, 48, wide, 64, 48);
        const double other[4] = {40, 41, 20.0, 15.0};
        warp(m, 64, 48, other, 41, 29);
        warp(m, 1, 1, K, 5, 4);
        warp(m, 3, 2, K, 7, 3);
        warp(m, 1, 1, K, 1, 1);
        calls += 6;
        if (m.id >= 2) {  // coefficients that overflow: +-1e300, inf - inf = NaN
            Model big = m;
            const int first = one_f ? 3 : 4;
            for (int k = first; k < m.n; ++k) big.p[k] = (k % 2 ? -1e300 : 1e300);
            warp(big, 64, 48, K, 64, 48);
            big.p[first] = 1.7e308;
            warp(big, 64, 48, wide, 64, 48);
            calls += 2;
        }
        // rejected arguments: nothing is read or written
        Model bad = m;
        bad.n = m.n + 1;
        warp(bad, 4, 4, K, 4, 4, APD_EINVAL);
        bad = m;
        bad.p[0] = 0.0;
        warp(bad, 4, 4, K, 4, 4, APD_EINVAL);
        bad = m;
        bad.p[m.n - 1] = NAN;
        warp(bad, 4, 4, K, 4, 4, APD_EINVAL);
        expect(apd_prep_undistort_bgr8_host(m.id, m.p, m.n, 0, 4, (const uint8_t *)"", K, 4, 4, (uint8_t *)&calls) == APD_EINVAL,
               "size 0");
        expect(apd_prep_undistort_bgr8_host(m.id, m.p, m.n, 4, 4, nullptr, K, 4, 4, nullptr) == APD_EINVAL, "NULL");

        // keypoints: in the image, far outside, and none
        const int n = 200;
        double *xy = (double *)std::malloc(sizeof(double) * 2 * n);
        double *out = (double *)std::malloc(sizeof(double) * 2 * n);
        for (int i = 0; i < n; ++i) {
            xy[2 * i] = (double)(next_u32() % 6400) / 100.0;
            xy[2 * i + 1] = (double)(next_u32() % 4800) / 100.0;
        }
        xy[0] = 1e9;
        xy[1] = -1e9;
        int64_t unresolved = -1;
        expect(apd_prep_undistort_xy(m.id, m.p, m.n, n, xy, out, &unresolved) == APD_OK, "undistort_xy");
        expect(unresolved >= 0 && unresolved <= n, "unresolved count");
        expect(apd_prep_undistort_xy(m.id, m.p, m.n, n, xy, xy, nullptr) == APD_OK, "undistort_xy in place");
        expect(apd_prep_undistort_xy(m.id, m.p, m.n, 0, nullptr, nullptr, &unresolved) == APD_OK && unresolved == 0, "n = 0");
        expect(apd_prep_undistort_xy(m.id, m.p, m.n - 1, n, xy, out, nullptr) == APD_EINVAL, "xy count");
        std::free(xy);
        std::free(out);
    }
    const Model fov = {7, 5, {50, 51, 30, 22, 0.9}};
    const double K[4] = {50, 51, 30, 22};
    warp(fov, 4, 4, K, 4, 4, APD_EINVAL);
    expect(apd_prep_atan_c(0.0) == 0.0 && apd_prep_atan_c(1.0) > 0.78 && apd_prep_atan_c(INFINITY) > 1.57, "atan_c");
    std::printf("undistort sanitizer run: %ld warps, %d failures\n", calls, g_fail);
    return g_fail ? 1 : 0;
}
