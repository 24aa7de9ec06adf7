// apd_undistort_host.cpp — the host-only entries of include/apd_prep.h's undistortion: the warp on
// the CPU (the device kernel's baseline and what the CPU tests run) and the keypoint inverse. No HIP
// call: it is part of libapd_hip.so and also builds alone (host/Makefile, sanitize-undistort).
// Compile with -ffp-contract=off.
#include <cmath>
#include <cstdint>

#include "../../include/apd_prep.h"
#include "apd_undistort.h"

namespace {

using namespace apd_ud;

template <int M>
void warp_all(const Warp &W) {
    for (int y = 0; y < W.oh; ++y)
        for (int x = 0; x < W.ow; ++x) warp_pixel<M>(W, x, y);
}

void forward_any(int model, const double *k, double u, double v, double &ud, double &vd) {
    switch (model) {
        case SIMPLE_PINHOLE: forward<SIMPLE_PINHOLE>(k, u, v, ud, vd); break;
        case PINHOLE: forward<PINHOLE>(k, u, v, ud, vd); break;
        case SIMPLE_RADIAL: forward<SIMPLE_RADIAL>(k, u, v, ud, vd); break;
        case RADIAL: forward<RADIAL>(k, u, v, ud, vd); break;
        case OPENCV: forward<OPENCV>(k, u, v, ud, vd); break;
        case OPENCV_FISHEYE: forward<OPENCV_FISHEYE>(k, u, v, ud, vd); break;
        case FULL_OPENCV: forward<FULL_OPENCV>(k, u, v, ud, vd); break;
        case SIMPLE_RADIAL_FISHEYE: forward<SIMPLE_RADIAL_FISHEYE>(k, u, v, ud, vd); break;
        case RADIAL_FISHEYE: forward<RADIAL_FISHEYE>(k, u, v, ud, vd); break;
        default: forward<THIN_PRISM_FISHEYE>(k, u, v, ud, vd); break;
    }
}

}  // namespace

extern "C" {

int32_t apd_prep_undistort_bgr8_host(int32_t model_id, const double *params, int32_t n_params, int32_t src_w,
                                     int32_t src_h, const uint8_t *src, const double *out_K, int32_t out_w,
                                     int32_t out_h, uint8_t *dst) {
    if (check_warp(model_id, params, n_params, src_w, src_h, src, out_K, out_w, out_h, dst)) return APD_EINVAL;
    Warp W;
    fill_warp(W, params, n_params, src_w, src_h, src, out_K, out_w, out_h, dst);
    switch (model_id) {
        case SIMPLE_PINHOLE: warp_all<SIMPLE_PINHOLE>(W); break;
        case PINHOLE: warp_all<PINHOLE>(W); break;
        case SIMPLE_RADIAL: warp_all<SIMPLE_RADIAL>(W); break;
        case RADIAL: warp_all<RADIAL>(W); break;
        case OPENCV: warp_all<OPENCV>(W); break;
        case OPENCV_FISHEYE: warp_all<OPENCV_FISHEYE>(W); break;
        case FULL_OPENCV: warp_all<FULL_OPENCV>(W); break;
        case SIMPLE_RADIAL_FISHEYE: warp_all<SIMPLE_RADIAL_FISHEYE>(W); break;
        case RADIAL_FISHEYE: warp_all<RADIAL_FISHEYE>(W); break;
        default: warp_all<THIN_PRISM_FISHEYE>(W); break;
    }
    return APD_OK;
}

double apd_prep_atan_c(double x) { return atan_c(x); }

int32_t apd_prep_undistort_xy(int32_t model_id, const double *params, int32_t n_params, int64_t n, const double *xy_in,
                              double *xy_out, int64_t *unresolved) {
    const int np = num_params(model_id);
    if (np == 0 || !params || n_params != np || n < 0 || (n > 0 && (!xy_in || !xy_out))) return APD_EINVAL;
    for (int i = 0; i < np; ++i)
        if (!std::isfinite(params[i])) return APD_EINVAL;
    const bool one_f = single_focal(model_id);
    const double fx = params[0], fy = one_f ? params[0] : params[1];
    const double cx = one_f ? params[1] : params[2], cy = one_f ? params[2] : params[3];
    if (!(fx > 0.0) || !(fy > 0.0)) return APD_EINVAL;
    const double *k = params + (one_f ? 3 : 4);
    const double h = 1e-6, tol = 1e-10;
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double tx = (xy_in[2 * i] - cx) / fx, ty = (xy_in[2 * i + 1] - cy) / fy;
        double u = tx, v = ty;
        bool done = false;
        for (int step = 0; step < 100 && std::isfinite(u) && std::isfinite(v); ++step) {
            double f0, f1, a0, b0, a1, b1, c0, d0, c1, d1;
            forward_any(model_id, k, u, v, f0, f1);
            forward_any(model_id, k, u - h, v, a0, b0);
            forward_any(model_id, k, u + h, v, a1, b1);
            forward_any(model_id, k, u, v - h, c0, d0);
            forward_any(model_id, k, u, v + h, c1, d1);
            const double j00 = (a1 - a0) / (2.0 * h), j10 = (b1 - b0) / (2.0 * h);
            const double j01 = (c1 - c0) / (2.0 * h), j11 = (d1 - d0) / (2.0 * h);
            const double e0 = f0 - tx, e1 = f1 - ty;
            const double det = j00 * j11 - j01 * j10;
            const double du = (j11 * e0 - j01 * e1) / det, dv = (j00 * e1 - j10 * e0) / det;
            u = u - du;
            v = v - dv;
            if (std::fabs(du) < tol && std::fabs(dv) < tol) {
                done = true;
                break;
            }
        }
        const double ox = fx * u + cx, oy = fy * v + cy;
        if (done && std::isfinite(ox) && std::isfinite(oy)) {
            xy_out[2 * i] = ox;
            xy_out[2 * i + 1] = oy;
        } else {
            xy_out[2 * i] = -1.0;
            xy_out[2 * i + 1] = -1.0;
            ++bad;
        }
    }
    if (unresolved) *unresolved = bad;
    return APD_OK;
}

}  // extern "C"
