// apd_register_host.cpp — the host twins of include/apd_eval.h's crop / nearest / transform /
// registration calls: one thread, no context, no device. They restate the contract with the shared
// statements of apd_register.h, so the device calls can be checked against them bit for bit.
// Compiled with -ffp-contract=off like the rest of the library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "apd_register.h"

namespace {

bool finite16(const double *T) {
    if (!T) return true;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return false;
    return true;
}

bool n_ok(int64_t n, const void *p) { return n >= 0 && n <= (int64_t)INT32_MAX && (n == 0 || p); }

// Nearest finite target under the tie rule: smallest (dx*dx + dy*dy) + dz*dz in fp32, the lowest index
// among equals. A uniform grid of cell just above max_dist when that is finite and the grid is of
// usable size, else brute force over all targets.
struct HostNN {
    const float *t = nullptr;
    int64_t nt = 0;
    bool grid = false;
    double lo[3] = {0, 0, 0}, cell = 0.0;
    int64_t dim[3] = {0, 0, 0};
    std::vector<std::pair<int64_t, int32_t>> cells;  // (cell key, target index), sorted
    std::vector<int32_t> finite;                     // brute force: the finite targets

    static bool fin3(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

    void build(int64_t n, const float *xyz, float max_dist) {
        t = xyz;
        nt = n;
        double hi[3] = {0, 0, 0};
        bool any = false;
        for (int64_t i = 0; i < n; ++i) {
            const float *p = xyz + 3 * i;
            if (!fin3(p)) continue;
            finite.push_back((int32_t)i);
            for (int a = 0; a < 3; ++a) {
                lo[a] = any ? std::min(lo[a], (double)p[a]) : (double)p[a];
                hi[a] = any ? std::max(hi[a], (double)p[a]) : (double)p[a];
            }
            any = true;
        }
        if (!any || !std::isfinite(max_dist) || !(max_dist > 0.0f) || finite.size() < 64) return;
        cell = (double)max_dist * 1.001;  // a target within max_dist (as computed in fp32) is in an adjacent cell
        double total = 1.0;
        for (int a = 0; a < 3; ++a) {
            const double d = std::floor((hi[a] - lo[a]) / cell) + 1.0;
            if (!(d < 2097152.0)) return;
            dim[a] = (int64_t)d;
            total *= d;
        }
        if (total < 8.0) return;  // nothing to gain
        cells.reserve(finite.size());
        for (int32_t i : finite) {
            const float *p = xyz + 3 * (int64_t)i;
            int64_t c[3];
            for (int a = 0; a < 3; ++a) c[a] = std::min((int64_t)std::floor(((double)p[a] - lo[a]) / cell), dim[a] - 1);
            cells.emplace_back((c[0] * dim[1] + c[1]) * dim[2] + c[2], i);
        }
        std::sort(cells.begin(), cells.end());
        grid = true;
    }

    static void offer(const float *t, int32_t j, float qx, float qy, float qz, float &cur, int32_t &best) {
        const float *p = t + 3 * (int64_t)j;
        const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < cur || (d2 == cur && j < best)) {
            cur = d2;
            best = j;
        }
    }

    // idx or -1, d2 = the minimal computed d2; the cut is sqrtf(d2) <= max_dist
    int32_t query(float qx, float qy, float qz, float max_dist, float &d2) const {
        const float inf = std::numeric_limits<float>::infinity();
        d2 = inf;
        if (!(std::isfinite(qx) && std::isfinite(qy) && std::isfinite(qz))) return -1;
        float cur = inf;
        int32_t best = std::numeric_limits<int32_t>::max();
        if (!grid) {
            for (int32_t j : finite) offer(t, j, qx, qy, qz, cur, best);
        } else {
            const float q[3] = {qx, qy, qz};
            int64_t c[3];
            for (int a = 0; a < 3; ++a) {
                const double f = std::floor(((double)q[a] - lo[a]) / cell);
                if (!(f >= -2.0 && f <= (double)dim[a] + 1.0)) return -1;  // farther than a cell from the box
                c[a] = (int64_t)f;
            }
            for (int64_t x = c[0] - 1; x <= c[0] + 1; ++x)
                for (int64_t y = c[1] - 1; y <= c[1] + 1; ++y)
                    for (int64_t z = c[2] - 1; z <= c[2] + 1; ++z) {
                        // the last cell of an axis also holds the points on the box's far face
                        if (x < 0 || y < 0 || z < 0 || x >= dim[0] || y >= dim[1] || z >= dim[2]) continue;
                        const int64_t key = (x * dim[1] + y) * dim[2] + z;
                        auto it = std::lower_bound(cells.begin(), cells.end(), std::make_pair(key, (int32_t)-1));
                        for (; it != cells.end() && it->first == key; ++it) offer(t, it->second, qx, qy, qz, cur, best);
                    }
        }
        if (best == std::numeric_limits<int32_t>::max()) return -1;
        if (!(sqrtf(cur) <= max_dist)) return -1;
        d2 = cur;
        return best;
    }
};

// the tree sum of the contract over per-point term rows
struct TreeSummer {
    std::vector<double> buf = std::vector<double>((size_t)APD_REG_BLOCK * APD_REG_SUMS);
    double total[APD_REG_SUMS];
    int64_t blocks = 0;
    int fill = 0;
    TreeSummer() {
        for (double &v : total) v = 0.0;
    }
    void push(const double *v) {
        for (int k = 0; k < APD_REG_SUMS; ++k) buf[(size_t)fill * APD_REG_SUMS + k] = v[k];
        if (++fill == APD_REG_BLOCK) flush();
    }
    void flush() {
        if (fill == 0) return;
        for (size_t i = (size_t)fill * APD_REG_SUMS; i < buf.size(); ++i) buf[i] = 0.0;
        for (int w = APD_REG_BLOCK; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i)
                for (int k = 0; k < APD_REG_SUMS; ++k)
                    buf[(size_t)i * APD_REG_SUMS + k] =
                        buf[(size_t)(2 * i) * APD_REG_SUMS + k] + buf[(size_t)(2 * i + 1) * APD_REG_SUMS + k];
        for (int k = 0; k < APD_REG_SUMS; ++k) total[k] = blocks == 0 ? buf[k] : total[k] + buf[k];
        ++blocks;
        fill = 0;
    }
};

void host_sums(const HostNN &nn, int64_t n, const float *xyz, const double *T, float max_corr, double *m) {
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!T) T = I;
    TreeSummer sum;
    for (int64_t i = 0; i < n; ++i) {
        double p[3], v[APD_REG_SUMS];
        apd_reg_xform(T, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], p);
        const float qx = (float)p[0], qy = (float)p[1], qz = (float)p[2];
        const bool fin = std::isfinite(qx) && std::isfinite(qy) && std::isfinite(qz);
        float d2 = 0.0f;
        const int32_t j = fin ? nn.query(qx, qy, qz, max_corr, d2) : -1;
        const float *t = j >= 0 ? nn.t + 3 * (int64_t)j : nullptr;
        apd_reg_terms(fin, j >= 0, qx, qy, qz, t ? t[0] : 0.0f, t ? t[1] : 0.0f, t ? t[2] : 0.0f, d2, v);
        sum.push(v);
    }
    sum.flush();
    for (int k = 0; k < APD_REG_SUMS; ++k) m[k] = sum.total[k];
}

}  // namespace

extern "C" {

int32_t apd_eval_crop_volume_host(int64_t n, const float *xyz, const double *T, int32_t axis, double axis_min,
                                  double axis_max, int32_t m, const double *poly, int32_t *keep_idx, int64_t *n_keep) {
    if (!n_ok(n, xyz) || !n_keep || (n > 0 && !keep_idx) || !poly || m < 3 || m > (1 << 20) || axis < 0 || axis > 2 ||
        !std::isfinite(axis_min) || !std::isfinite(axis_max) || !finite16(T))
        return APD_EINVAL;
    for (int i = 0; i < 2 * m; ++i)
        if (!std::isfinite(poly[i])) return APD_EINVAL;
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i)
        if (apd_reg_crop_keep(T, axis, axis_min, axis_max, m, poly, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]))
            keep_idx[k++] = (int32_t)i;
    *n_keep = k;
    return APD_OK;
}

int32_t apd_eval_nearest_host(int64_t nt, const float *target, int64_t n, const float *xyz, float max_dist,
                              float *dist, int32_t *idx) {
    if (!n_ok(nt, target) || !n_ok(n, xyz) || !(max_dist >= 0.0f)) return APD_EINVAL;
    HostNN nn;
    nn.build(nt, target, max_dist);
    for (int64_t i = 0; i < n; ++i) {
        float d2;
        const int32_t j = nn.query(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], max_dist, d2);
        if (dist) dist[i] = j >= 0 ? sqrtf(d2) : std::numeric_limits<float>::infinity();
        if (idx) idx[i] = j;
    }
    return APD_OK;
}

int32_t apd_eval_transform_host(int64_t n, const float *xyz, const double *T, float *out) {
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!n_ok(n, xyz) || (n > 0 && !out) || !finite16(T)) return APD_EINVAL;
    if (!T) T = I;
    for (int64_t i = 0; i < n; ++i) {
        double p[3];
        apd_reg_xform(T, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], p);
        for (int a = 0; a < 3; ++a) out[3 * i + a] = (float)p[a];
    }
    return APD_OK;
}

int32_t apd_eval_register_sums_host(int64_t nt, const float *target, int64_t n, const float *xyz, const double *T,
                                    float max_corr, double *sums) {
    if (!n_ok(nt, target) || !n_ok(n, xyz) || !sums || !finite16(T) || !(max_corr > 0.0f) || !std::isfinite(max_corr))
        return APD_EINVAL;
    HostNN nn;
    nn.build(nt, target, max_corr);
    host_sums(nn, n, xyz, T, max_corr, sums);
    return APD_OK;
}

int32_t apd_eval_register_host(int64_t nt, const float *target, int64_t n, const float *xyz, const double *T0,
                               float max_corr, int32_t with_scale, int32_t max_iter, double eps_fitness,
                               double eps_rmse, double *T, apd_eval_reg_info *info) {
    if (!n_ok(nt, target) || !n_ok(n, xyz) || !T || !info || !finite16(T0) || !(max_corr > 0.0f) ||
        !std::isfinite(max_corr) || with_scale < 0 || with_scale > 1 || max_iter < 1 || max_iter > 1000 ||
        !(eps_fitness >= 0.0) || !(eps_rmse >= 0.0))
        return APD_EINVAL;
    HostNN nn;
    nn.build(nt, target, max_corr);
    return apd_reg_iterate(T0, with_scale, max_iter, eps_fitness, eps_rmse, T, info, [&](const double *cur, double *m) {
        host_sums(nn, n, xyz, cur, max_corr, m);
        return (int32_t)APD_OK;
    });
}

}  // extern "C"
