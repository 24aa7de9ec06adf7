// apd_undistort.h — the arithmetic of include/apd_prep.h's "Undistortion" section, one text for the
// host (apd_undistort_host.cpp) and the device (k_pr_undistort in apd_prep.hip): atan_c, the forward
// distortion functions of COLMAP's camera models and the 1/256 fixed-point bilinear sample with a
// black border. IEEE double, every sum and product as written; whatever compiles this file does so
// with -ffp-contract=off.
#ifndef APD_UNDISTORT_H_
#define APD_UNDISTORT_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APD_UD_HD __host__ __device__ __forceinline__
#else
#define APD_UD_HD inline
#endif

namespace apd_ud {

enum {
    SIMPLE_PINHOLE = 0, PINHOLE = 1, SIMPLE_RADIAL = 2, RADIAL = 3, OPENCV = 4, OPENCV_FISHEYE = 5, FULL_OPENCV = 6,
    FOV = 7, SIMPLE_RADIAL_FISHEYE = 8, RADIAL_FISHEYE = 9, THIN_PRISM_FISHEYE = 10
};
constexpr int MAX_PARAMS = 12;

// parameters of a model, 0 for an unknown or unsupported one (FOV)
APD_UD_HD int num_params(int model) {
    switch (model) {
        case SIMPLE_PINHOLE: return 3;
        case PINHOLE: return 4;
        case SIMPLE_RADIAL: return 4;
        case RADIAL: return 5;
        case OPENCV: return 8;
        case OPENCV_FISHEYE: return 8;
        case FULL_OPENCV: return 12;
        case SIMPLE_RADIAL_FISHEYE: return 4;
        case RADIAL_FISHEYE: return 5;
        case THIN_PRISM_FISHEYE: return 12;
        default: return 0;
    }
}
// models whose parameters start f cx cy (the others: fx fy cx cy)
APD_UD_HD bool single_focal(int model) {
    return model == SIMPLE_PINHOLE || model == SIMPLE_RADIAL || model == RADIAL || model == SIMPLE_RADIAL_FISHEYE ||
           model == RADIAL_FISHEYE;
}

// The arctangent of x >= 0 (a NaN comes back as a NaN) by the contract's reduction and polynomial.
APD_UD_HD double atan_c(double x) {
    if (x >= 73786976294838206464.0) return 1.57079632679489655800e+00 + 6.12323399573676603587e-17;  // 2^66
    double hi = 0.0, lo = 0.0;
    bool reduced = true;
    if (x < 0.4375) {
        if (x < 1.862645149230957e-09) return x;  // 2^-29
        reduced = false;
    } else if (x < 1.1875) {
        if (x < 0.6875) {
            hi = 4.63647609000806093515e-01;
            lo = 2.26987774529616870924e-17;
            x = (2.0 * x - 1.0) / (2.0 + x);
        } else {
            hi = 7.85398163397448278999e-01;
            lo = 3.06161699786838301793e-17;
            x = (x - 1.0) / (x + 1.0);
        }
    } else if (x < 2.4375) {
        hi = 9.82793723247329054082e-01;
        lo = 1.39033110312309984516e-17;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        hi = 1.57079632679489655800e+00;
        lo = 6.12323399573676603587e-17;
        x = -1.0 / x;
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 +
                           w * (1.42857142725034663711e-01 +
                                w * (9.09088713343650656196e-02 +
                                     w * (6.66107313738753120669e-02 +
                                          w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 +
                           w * (-1.11111104054623557880e-01 +
                                w * (-7.69187620504482999495e-02 +
                                     w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (!reduced) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}

// normalised pinhole (u, v) -> normalised distorted (ud, vd). k: the model's parameters after the
// intrinsics (k = params + 3 for the f cx cy models, params + 4 for the others).
template <int M>
APD_UD_HD void forward(const double *k, double u, double v, double &ud, double &vd) {
    if constexpr (M == SIMPLE_PINHOLE || M == PINHOLE) {
        ud = u;
        vd = v;
    } else if constexpr (M == SIMPLE_RADIAL || M == RADIAL || M == OPENCV || M == FULL_OPENCV) {
        const double r2 = u * u + v * v;
        if constexpr (M == SIMPLE_RADIAL) {
            const double rad = k[0] * r2;
            ud = u + u * rad;
            vd = v + v * rad;
        } else if constexpr (M == RADIAL) {
            const double rad = k[0] * r2 + (k[1] * r2) * r2;
            ud = u + u * rad;
            vd = v + v * rad;
        } else if constexpr (M == OPENCV) {
            const double rad = k[0] * r2 + (k[1] * r2) * r2;
            ud = u + ((u * rad + ((2.0 * k[2]) * u) * v) + k[3] * (r2 + (2.0 * u) * u));
            vd = v + ((v * rad + ((2.0 * k[3]) * u) * v) + k[2] * (r2 + (2.0 * v) * v));
        } else {  // FULL_OPENCV: k1 k2 p1 p2 k3 k4 k5 k6
            const double g = (1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))) / (1.0 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])));
            ud = (u * g + ((2.0 * k[2]) * u) * v) + k[3] * (r2 + (2.0 * u) * u);
            vd = (v * g + ((2.0 * k[3]) * u) * v) + k[2] * (r2 + (2.0 * v) * v);
        }
    } else {  // the fisheye family
        const double r2 = u * u + v * v;
        const double r = sqrt(r2);
        const double s = r2 == 0.0 ? 1.0 : atan_c(r) / r;
        const double a = u * s, b = v * s;
        const double t2 = a * a + b * b;
        if constexpr (M == SIMPLE_RADIAL_FISHEYE) {
            const double rad = k[0] * t2;
            ud = a + a * rad;
            vd = b + b * rad;
        } else if constexpr (M == RADIAL_FISHEYE) {
            const double rad = k[0] * t2 + (k[1] * t2) * t2;
            ud = a + a * rad;
            vd = b + b * rad;
        } else if constexpr (M == OPENCV_FISHEYE) {
            const double rad = t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])));
            ud = a + a * rad;
            vd = b + b * rad;
        } else {  // THIN_PRISM_FISHEYE: k1 k2 p1 p2 k3 k4 sx1 sy1
            const double rad = t2 * (k[0] + t2 * (k[1] + t2 * (k[4] + t2 * k[5])));
            ud = a + (((a * rad + ((2.0 * k[2]) * a) * b) + k[3] * (t2 + (2.0 * a) * a)) + k[6] * t2);
            vd = b + (((b * rad + ((2.0 * k[3]) * a) * b) + k[2] * (t2 + (2.0 * b) * b)) + k[7] * t2);
        }
    }
}

// The camera and the images of one warp. On the device it is a kernel argument, so every read of it
// is a scalar load.
struct Warp {
    double p[MAX_PARAMS];        // the source camera's parameters, in the model's order
    double ofx, ofy, ocx, ocy;   // the output camera
    const uint8_t *src;
    uint8_t *dst;
    int32_t sw, sh, ow, oh;
};

// output pixel (x, y) of the warp: 3 bytes at dst[(y*ow + x)*3]
template <int M>
APD_UD_HD void warp_pixel(const Warp &W, int x, int y) {
    constexpr bool one_f = M == SIMPLE_PINHOLE || M == SIMPLE_RADIAL || M == RADIAL || M == SIMPLE_RADIAL_FISHEYE ||
                           M == RADIAL_FISHEYE;
    const double fx = W.p[0], fy = one_f ? W.p[0] : W.p[1];
    const double cx = one_f ? W.p[1] : W.p[2], cy = one_f ? W.p[2] : W.p[3];
    const double u = (((double)x + 0.5) - W.ocx) / W.ofx;
    const double v = (((double)y + 0.5) - W.ocy) / W.ofy;
    double ud, vd;
    forward<M>(W.p + (one_f ? 3 : 4), u, v, ud, vd);
    const double sx = (fx * ud + cx) - 0.5;
    const double sy = (fy * vd + cy) - 0.5;
    uint8_t *o = W.dst + ((size_t)y * (size_t)W.ow + (size_t)x) * 3;
    if (!(sx > -1.0 && sx < (double)W.sw && sy > -1.0 && sy < (double)W.sh)) {
        o[0] = 0;
        o[1] = 0;
        o[2] = 0;
        return;
    }
    const double fxi = floor(sx), fyi = floor(sy);
    const int ix = (int)fxi, iy = (int)fyi;  // -1 .. size - 1
    const uint32_t wx = (uint32_t)(int)floor((sx - fxi) * 256.0 + 0.5);
    const uint32_t wy = (uint32_t)(int)floor((sy - fyi) * 256.0 + 0.5);
    const bool x0 = ix >= 0, x1 = ix + 1 < W.sw, y0 = iy >= 0, y1 = iy + 1 < W.sh;
    const uint8_t *r0 = W.src + ((size_t)(y0 ? iy : 0) * (size_t)W.sw) * 3;
    const uint8_t *r1 = W.src + ((size_t)(y1 ? iy + 1 : 0) * (size_t)W.sw) * 3;
    const size_t c0 = (size_t)(x0 ? ix : 0) * 3, c1 = (size_t)(x1 ? ix + 1 : 0) * 3;
    const uint32_t w00 = (256u - wx) * (256u - wy), w10 = wx * (256u - wy), w01 = (256u - wx) * wy, w11 = wx * wy;
    for (int c = 0; c < 3; ++c) {
        const uint32_t t00 = (x0 && y0) ? r0[c0 + c] : 0u, t10 = (x1 && y0) ? r0[c1 + c] : 0u;
        const uint32_t t01 = (x0 && y1) ? r1[c0 + c] : 0u, t11 = (x1 && y1) ? r1[c1 + c] : 0u;
        o[c] = (uint8_t)((t00 * w00 + t10 * w10 + t01 * w01 + t11 * w11 + 32768u) >> 16);
    }
}

// Host: what is wrong with the arguments of a warp (APD_EINVAL), or NULL
inline const char *check_warp(int model, const double *params, int n_params, int sw, int sh, const void *src,
                              const double *out_K, int ow, int oh, const void *dst) {
    const int np = num_params(model);
    if (np == 0) return "unknown or unsupported camera model";
    if (!params || !src || !out_K || !dst) return "a NULL pointer";
    if (n_params != np) return "n_params is not the model's parameter count";
    for (int i = 0; i < np; ++i)
        if (!(params[i] - params[i] == 0.0)) return "a non-finite camera parameter";
    for (int i = 0; i < 4; ++i)
        if (!(out_K[i] - out_K[i] == 0.0)) return "a non-finite output camera";
    if (!(params[0] > 0.0) || (!single_focal(model) && !(params[1] > 0.0))) return "a focal length that is not positive";
    if (!(out_K[0] > 0.0) || !(out_K[1] > 0.0)) return "an output focal length that is not positive";
    if (sw < 1 || sh < 1 || sw > 65536 || sh > 65536 || ow < 1 || oh < 1 || ow > 65536 || oh > 65536)
        return "an image size outside 1..65536";
    return nullptr;
}

inline void fill_warp(Warp &W, const double *params, int n_params, int sw, int sh, const uint8_t *src,
                      const double *out_K, int ow, int oh, uint8_t *dst) {
    for (int i = 0; i < MAX_PARAMS; ++i) W.p[i] = i < n_params ? params[i] : 0.0;
    W.ofx = out_K[0];
    W.ofy = out_K[1];
    W.ocx = out_K[2];
    W.ocy = out_K[3];
    W.src = src;
    W.dst = dst;
    W.sw = sw;
    W.sh = sh;
    W.ow = ow;
    W.oh = oh;
}

}  // namespace apd_ud

#endif  // APD_UNDISTORT_H_
