// apd_dtu_host.cpp — the host twins of include/apd_eval.h's radius thinning, observability mask,
// half-space and masked statistics: one thread, no context, no device. They restate the contract with
// the shared statements of apd_dtu.h, so the device calls can be checked against them bit for bit.
// Compiled with -ffp-contract=off like the rest of the library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "apd_dtu.h"

namespace {

bool n_ok(int64_t n, const void *p) { return n >= 0 && n <= (int64_t)INT32_MAX && (n == 0 || p); }

}  // namespace

extern "C" {

// The loop of the contract, literally: the finite points in ascending key; a point is kept iff no
// point kept before it is close. The grid (cell 2*radius, apd_dtu_cell) holds the kept points only
// and serves to find candidates; every decision is the d2 <= r2 test.
int32_t apd_eval_radius_thin_host(int64_t n, const float *xyz, float radius, const uint32_t *rank, int32_t *keep_idx,
                                  int64_t *n_keep) {
    float r2;
    double cell;
    if (!n_ok(n, xyz) || !n_keep || (n > 0 && !keep_idx) || !apd_dtu_radius(radius, &r2, &cell)) return APD_EINVAL;
    std::vector<int32_t> order;
    order.reserve((size_t)n);
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const float *p = xyz + 3 * i;
        if (!apd_dtu_finite3(p[0], p[1], p[2])) continue;
        for (int a = 0; a < 3; ++a) {
            const double c = apd_dtu_cell(p[a], cell);
            lo[a] = order.empty() ? c : std::min(lo[a], c);
            hi[a] = order.empty() ? c : std::max(hi[a], c);
        }
        order.push_back((int32_t)i);
    }
    *n_keep = 0;
    if (order.empty()) return APD_OK;
    for (int a = 0; a < 3; ++a)
        if (!(hi[a] - lo[a] < APD_DTU_CELL_SPAN)) return APD_EINVAL;
    if (rank)  // ascending (rank, index): the indices went in ascending and the sort is stable
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return rank[a] < rank[b]; });
    std::unordered_map<uint64_t, std::vector<int32_t>> grid;
    grid.reserve(order.size());
    std::vector<uint8_t> kept((size_t)n, 0);
    for (int32_t i : order) {
        const float *p = xyz + 3 * (int64_t)i;
        int64_t c[3];
        for (int a = 0; a < 3; ++a) c[a] = (int64_t)(apd_dtu_cell(p[a], cell) - lo[a]);
        bool keep = true;
        for (int64_t z = c[2] - 1; keep && z <= c[2] + 1; ++z)
            for (int64_t y = c[1] - 1; keep && y <= c[1] + 1; ++y)
                for (int64_t x = c[0] - 1; keep && x <= c[0] + 1; ++x) {
                    if (x < 0 || y < 0 || z < 0 || x >= (1 << 21) || y >= (1 << 21) || z >= (1 << 21)) continue;
                    const auto it = grid.find((uint64_t)z << 42 | (uint64_t)y << 21 | (uint64_t)x);
                    if (it == grid.end()) continue;
                    for (int32_t j : it->second) {
                        const float *q = xyz + 3 * (int64_t)j;
                        if (apd_dtu_close(p[0], p[1], p[2], q[0], q[1], q[2], r2)) {
                            keep = false;
                            break;
                        }
                    }
                }
        if (keep) {
            kept[(size_t)i] = 1;
            grid[(uint64_t)c[2] << 42 | (uint64_t)c[1] << 21 | (uint64_t)c[0]].push_back(i);
        }
    }
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i)
        if (kept[(size_t)i]) keep_idx[k++] = (int32_t)i;
    *n_keep = k;
    return APD_OK;
}

int32_t apd_eval_dtu_ranks(int64_t n, uint32_t seed, uint32_t *rank) {
    if (!n_ok(n, rank)) return APD_EINVAL;
    for (int64_t i = 0; i < n; ++i) rank[i] = apd_dtu_rank((uint32_t)i, seed);
    return APD_OK;
}

int32_t apd_eval_obs_mask_host(int64_t n, const float *xyz, const int32_t dims[3], const double origin[3], double res,
                               const uint8_t *mask, uint8_t *inside) {
    if (!n_ok(n, xyz) || (n > 0 && !inside) || !dims || !origin || !mask || !(res > 0.0) || !std::isfinite(res))
        return APD_EINVAL;
    apd_dtu_mask_geom g;
    double total = 1.0;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 1 || !std::isfinite(origin[k])) return APD_EINVAL;
        g.dims[k] = dims[k];
        g.origin[k] = origin[k];
        total *= (double)dims[k];
    }
    if (total > 2147483648.0) return APD_EINVAL;
    g.res = res;
    for (int64_t i = 0; i < n; ++i)
        inside[i] = apd_dtu_inside(g, mask, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) ? 1 : 0;
    return APD_OK;
}

int32_t apd_eval_half_space_host(int64_t n, const float *xyz, const double P[4], uint8_t *above) {
    if (!n_ok(n, xyz) || (n > 0 && !above) || !P) return APD_EINVAL;
    for (int64_t i = 0; i < n; ++i) above[i] = apd_dtu_above(P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) ? 1 : 0;
    return APD_OK;
}

int32_t apd_eval_masked_stats_host(int64_t n, const float *dist, const uint8_t *flag, float limit, int64_t *count,
                                   double *sum, double *median) {
    if (!n_ok(n, dist) || limit != limit) return APD_EINVAL;
    std::vector<float> sel;
    std::vector<double> buf((size_t)APD_EVAL_REG_BLOCK);
    double total = 0.0;
    for (int64_t b = 0; b < n; b += APD_EVAL_REG_BLOCK) {
        for (int64_t k = 0; k < APD_EVAL_REG_BLOCK; ++k) {
            const int64_t i = b + k;
            const bool s = i < n && apd_dtu_selected(dist[i], !flag || flag[i] != 0, limit);
            buf[(size_t)k] = s ? (double)dist[i] : 0.0;
            if (s) sel.push_back(dist[i]);
        }
        for (int w = APD_EVAL_REG_BLOCK; w > 1; w >>= 1)
            for (int k = 0; k < w / 2; ++k) buf[(size_t)k] = buf[(size_t)(2 * k)] + buf[(size_t)(2 * k + 1)];
        total = b == 0 ? buf[0] : total + buf[0];
    }
    std::sort(sel.begin(), sel.end(), [](float a, float b) { return apd_dtu_ord(a) < apd_dtu_ord(b); });
    const size_t m = sel.size();
    if (count) *count = (int64_t)m;
    if (sum) *sum = total;
    if (median) *median = m == 0 ? 0.0 : (m & 1) ? (double)sel[(m - 1) / 2] : ((double)sel[m / 2 - 1] + (double)sel[m / 2]) / 2.0;
    return APD_OK;
}

}  // extern "C"
