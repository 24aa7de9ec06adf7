// apd_dtu.h — the parts of the DTU contract (include/apd_eval.h, last section) that the device code
// (apd_eval.hip) and the host twins (apd_dtu_host.cpp) must state identically: the close test, the
// candidate cell, the mask rule, the half-space, the selection of the statistics and the rank
// generator. Every translation unit that includes it is compiled with -ffp-contract=off.
#ifndef APD_DTU_H_
#define APD_DTU_H_

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/apd_eval.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APD_DTU_HD __host__ __device__ __forceinline__
#else
#define APD_DTU_HD inline
#endif

#define APD_DTU_CELL_SPAN 2097152.0 /* 2^21 cells per axis: three fields of a 63-bit key */

// close iff d2 <= r2, the distance contract's d2
APD_DTU_HD bool apd_dtu_close(float ax, float ay, float az, float bx, float by, float bz, float r2) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= r2;
}

// The candidate cell of a coordinate, cell = 2.0 * (double)radius. Two close points lie in the same
// or in adjacent cells on every axis:
//   close => fl(dx*dx) <= r2, both normal or dx*dx below the normal range => |dx| <= radius (1 + 2^-22)
//   => |x_i - x_j| <= radius (1 + 2^-21) = t, the subtraction's own rounding included.
//   If max(|x_i|, |x_j|) / cell > 2^24 the spacing of fp32 there exceeds cell > t, so x_i = x_j and the
//   cells coincide. Otherwise both double quotients err by at most 2^24 * 2^-53 = 2^-29 and differ by
//   at most t / cell + 2^-28 < 1, so their floors differ by at most 1.
APD_DTU_HD double apd_dtu_cell(float x, double cell) { return floor((double)x / cell); }

// r2 and the cell size of a radius; false for a radius the contract rejects
inline bool apd_dtu_radius(float radius, float *r2, double *cell) {
    const float p = radius * radius;
    uint32_t u;
    memcpy(&u, &p, 4);
    const uint32_t e = (u >> 23) & 0xFFu;
    if (!(radius > 0.0f) || e == 0u || e == 0xFFu) return false;  // r2 zero, subnormal, inf or NaN
    *r2 = p;
    *cell = 2.0 * (double)radius;
    return true;
}

APD_DTU_HD bool apd_dtu_finite3(float x, float y, float z) {
    return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;
}

// the mask rule for one point
struct apd_dtu_mask_geom {
    int32_t dims[3];
    double origin[3];
    double res;
};
APD_DTU_HD bool apd_dtu_inside(const apd_dtu_mask_geom &g, const uint8_t *mask, float x, float y, float z) {
    if (!apd_dtu_finite3(x, y, z)) return false;
    const float p[3] = {x, y, z};
    int64_t v[3];
    for (int k = 0; k < 3; ++k) {
        const double t = round(((double)p[k] - g.origin[k]) / g.res + 1.0);
        if (!(t >= 1.0 && t <= (double)g.dims[k])) return false;
        v[k] = (int64_t)t - 1;
    }
    return mask[v[0] + (int64_t)g.dims[0] * (v[1] + (int64_t)g.dims[1] * v[2])] != 0;
}

APD_DTU_HD bool apd_dtu_above(const double *P, float x, float y, float z) {
    return ((P[0] * (double)x + P[1] * (double)y) + P[2] * (double)z) + P[3] > 0.0;
}

// the selection of the masked statistics
APD_DTU_HD bool apd_dtu_selected(float d, bool flagged, float limit) {
    return flagged && d <= limit && d - d == 0.0f;
}

// order-preserving uint32 image of a float (sign-magnitude order, -0 < +0)
APD_DTU_HD uint32_t apd_dtu_ord(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t u = __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// word 0 of Philox4x32-10 with counter (i, 0, 0, 0) and key (seed, 0): csrc/apd_device.h's rounds
APD_DTU_HD uint32_t apd_dtu_rank(uint32_t i, uint32_t seed) {
    uint32_t x0 = i, x1 = 0u, x2 = 0u, x3 = 0u, key0 = seed, key1 = 0u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32);
        const uint32_t lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
        const uint32_t n0 = hi1 ^ x1 ^ key0, n2 = hi0 ^ x3 ^ key1;
        x0 = n0; x1 = lo1; x2 = n2; x3 = lo0;
        key0 += 0x9E3779B9u; key1 += 0xBB67AE85u;
    }
    return x0;
}

#endif  // APD_DTU_H_
