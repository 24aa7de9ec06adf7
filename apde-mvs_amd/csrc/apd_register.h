// apd_register.h — the parts of the registration / crop contract (include/apd_eval.h, last section)
// that the device code (apd_eval.hip) and the host twins (apd_register_host.cpp) must state
// identically: the double transform and its fp32 rounding, the crop rule, the moment layout, the
// Umeyama solve with its own 3x3 Jacobi SVD, and the iteration loop around a moments provider.
// Every translation unit that includes it is compiled with -ffp-contract=off.
#ifndef APD_REGISTER_H_
#define APD_REGISTER_H_

#include <math.h>
#include <stdint.h>

#include "../../include/apd_eval.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APD_REG_HD __host__ __device__ __forceinline__
#else
#define APD_REG_HD inline
#endif

#define APD_REG_BLOCK 1024  /* source indices per summation block (APD_EVAL_REG_BLOCK) */
#define APD_REG_SUMS 19     /* 17 moments, the squared-distance sum, the finite count */
/* layout of the sums: 0 count | 1..3 sum q | 4..6 sum t | 7..15 sum q_a t_b (index 7 + 3a + b) |
   16 sum |q|^2 | 17 sum d2 | 18 number of source points whose q is finite */

// p' = T (x, y, z, 1), rows 0..2, in double, left to right
APD_REG_HD void apd_reg_xform(const double *T, float x, float y, float z, double p[3]) {
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    for (int r = 0; r < 3; ++r) p[r] = ((T[4 * r] * dx + T[4 * r + 1] * dy) + T[4 * r + 2] * dz) + T[4 * r + 3];
}

APD_REG_HD bool apd_reg_finite(double v) { return v - v == 0.0; }
APD_REG_HD bool apd_reg_finitef(float v) { return v - v == 0.0f; }

// the crop rule for one point; poly = m (u, v) pairs
APD_REG_HD bool apd_reg_crop_keep(const double *T, int axis, double axis_min, double axis_max, int m,
                                  const double *poly, float x, float y, float z) {
    if (!(apd_reg_finitef(x) && apd_reg_finitef(y) && apd_reg_finitef(z))) return false;
    double p[3];
    if (T) {
        apd_reg_xform(T, x, y, z, p);
    } else {
        p[0] = (double)x;
        p[1] = (double)y;
        p[2] = (double)z;
    }
    if (!(apd_reg_finite(p[0]) && apd_reg_finite(p[1]) && apd_reg_finite(p[2]))) return false;
    const int ui = axis == 0 ? 1 : 0, vi = axis == 2 ? 1 : 2;
    const double pu = p[ui], pv = p[vi], pw = p[axis];
    if (!(axis_min <= pw && pw <= axis_max)) return false;
    bool odd = false;
    for (int i = 0; i < m; ++i) {
        const int j = i + 1 == m ? 0 : i + 1;
        const double Ui = poly[2 * i], Vi = poly[2 * i + 1], Uj = poly[2 * j], Vj = poly[2 * j + 1];
        if ((Vi > pv) != (Vj > pv) && pu < ((Uj - Ui) * (pv - Vi)) / (Vj - Vi) + Ui) odd = !odd;
    }
    return odd;
}

// the 19 terms of one source point with transformed position q (already rounded to fp32), its
// correspondence t and their squared distance d2; has = false: every moment term is +0.0
APD_REG_HD void apd_reg_terms(bool q_finite, bool has, float qx, float qy, float qz, float tx, float ty, float tz,
                              float d2, double v[APD_REG_SUMS]) {
    for (int k = 0; k < APD_REG_SUMS; ++k) v[k] = 0.0;
    v[18] = q_finite ? 1.0 : 0.0;
    if (!has) return;
    const double q[3] = {(double)qx, (double)qy, (double)qz}, t[3] = {(double)tx, (double)ty, (double)tz};
    v[0] = 1.0;
    for (int a = 0; a < 3; ++a) {
        v[1 + a] = q[a];
        v[4 + a] = t[a];
        for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] = q[a] * t[b];
    }
    v[16] = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    v[17] = (double)d2;
}

// ---- host only from here (plain inline functions) ----

// C = A B, 4x4 row-major
inline void apd_reg_mul4(const double *A, const double *B, double *C) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
            r[4 * i + j] = s;
        }
    for (int i = 0; i < 16; ++i) C[i] = r[i];
}

// A = U diag(d) V^T by one-sided Jacobi rotations (Hestenes), d descending and >= 0. A zero
// singular value leaves its column of U to be completed: u2 = u0 x u1 (its sign does not matter to
// the caller, who multiplies by det(U V^T)). Returns the rank found (0..3).
inline int apd_reg_svd3(const double A[9], double U[9], double d[3], double V[9]) {
    double B[9];  // columns are rotated until orthogonal
    for (int i = 0; i < 9; ++i) {
        B[i] = A[i];
        V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int r = 0; r < 3; ++r) {
                    alpha += B[3 * r + p] * B[3 * r + p];
                    beta += B[3 * r + q] * B[3 * r + q];
                    gamma += B[3 * r + p] * B[3 * r + q];
                }
                if (gamma == 0.0 || !(fabs(gamma) > 1e-300)) continue;
                const double lim = 1e-15 * sqrt(alpha * beta);
                if (fabs(gamma) <= lim) continue;
                off = fmax(off, fabs(gamma) / sqrt(alpha * beta));
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double bp = B[3 * r + p], bq = B[3 * r + q];
                    B[3 * r + p] = c * bp - s * bq;
                    B[3 * r + q] = s * bp + c * bq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - s * vq;
                    V[3 * r + q] = s * vp + c * vq;
                }
            }
        if (off == 0.0) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt((B[c] * B[c] + B[3 + c] * B[3 + c]) + B[6 + c] * B[6 + c]);
    for (int a = 0; a < 2; ++a)  // descending, stable
        for (int b = 0; b < 2 - a; ++b)
            if (nrm[ord[b]] < nrm[ord[b + 1]]) {
                const int t = ord[b];
                ord[b] = ord[b + 1];
                ord[b + 1] = t;
            }
    double Vs[9];
    int rank = 0;
    const double tiny = nrm[ord[0]] * 1e-14;
    for (int c = 0; c < 3; ++c) {
        const int s = ord[c];
        d[c] = nrm[s];
        for (int r = 0; r < 3; ++r) {
            Vs[3 * r + c] = V[3 * r + s];
            U[3 * r + c] = nrm[s] > tiny ? B[3 * r + s] / nrm[s] : 0.0;
        }
        if (nrm[s] > tiny) ++rank;
    }
    for (int i = 0; i < 9; ++i) V[i] = Vs[i];
    if (rank == 2) {
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
        d[2] = 0.0;
    }
    return rank;
}

inline double apd_reg_det3(const double *M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama from the sums: S (4x4, row-major) maps the q of the correspondences onto their t.
// false: fewer than 3 correspondences, a covariance of rank < 2, or (with_scale) no spread in q.
inline bool apd_reg_solve(const double *m, int with_scale, double S[16]) {
    const double N = m[0];
    if (!(N >= 3.0)) return false;
    double mq[3], mt[3], C[9];
    for (int a = 0; a < 3; ++a) {
        mq[a] = m[1 + a] / N;
        mt[a] = m[4 + a] / N;
    }
    // C[a][b] = E[t_a q_b] - mt_a mq_b   (rows: target, columns: source)
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] = m[7 + 3 * b + a] / N - mt[a] * mq[b];
    const double var_q = m[16] / N - ((mq[0] * mq[0] + mq[1] * mq[1]) + mq[2] * mq[2]);
    double U[9], d[3], V[9];
    if (apd_reg_svd3(C, U, d, V) < 2) return false;
    double UVt[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            UVt[3 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + U[3 * i + 2] * V[3 * j + 2];
    const double sg = apd_reg_det3(UVt) < 0.0 ? -1.0 : 1.0;
    double R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + sg * (U[3 * i + 2] * V[3 * j + 2]);
    double s = 1.0;
    if (with_scale) {
        if (!(var_q > 0.0)) return false;
        s = ((d[0] + d[1]) + sg * d[2]) / var_q;
        if (!(s > 0.0) || !apd_reg_finite(s)) return false;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) S[4 * i + j] = s * R[3 * i + j];
        S[4 * i + 3] = mt[i] - s * ((R[3 * i] * mq[0] + R[3 * i + 1] * mq[1]) + R[3 * i + 2] * mq[2]);
    }
    S[12] = S[13] = S[14] = 0.0;
    S[15] = 1.0;
    return true;
}

inline void apd_reg_fill_info(const double *m, int iterations, apd_eval_reg_info *info) {
    info->iterations = iterations;
    info->reserved = 0;
    info->n_corr = (int64_t)m[0];
    info->n_finite = (int64_t)m[18];
    info->fitness = m[18] > 0.0 ? m[0] / m[18] : 0.0;
    info->rmse = m[0] > 0.0 ? sqrt(m[17] / m[0]) : 0.0;
}

// The iteration loop of apd_eval_register. sums(T, m) evaluates the 19 sums under T and returns
// APD_OK or a status that ends the call. The transform is evaluated once more after the last update,
// so info always describes the returned T (except on APD_ESTATE, see the header).
template <class Sums>
inline int32_t apd_reg_iterate(const double *T0, int with_scale, int max_iter, double eps_fitness, double eps_rmse,
                               double T[16], apd_eval_reg_info *info, Sums sums) {
    double cur[16], valid[16];
    for (int i = 0; i < 16; ++i) cur[i] = T0 ? T0[i] : (i % 5 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 16; ++i) valid[i] = cur[i];
    apd_eval_reg_info prev{};
    int it = 0;
    for (;;) {
        double m[APD_REG_SUMS];
        const int32_t st = sums(cur, m);
        if (st != APD_OK) return st;
        apd_reg_fill_info(m, it, info);
        double S[16];
        if (info->n_corr < 3) break;
        for (int i = 0; i < 16; ++i) valid[i] = cur[i];
        if (it > 0 && fabs(info->fitness - prev.fitness) < eps_fitness && fabs(info->rmse - prev.rmse) < eps_rmse) {
            for (int i = 0; i < 16; ++i) T[i] = cur[i];
            return APD_OK;
        }
        if (it == max_iter) {
            for (int i = 0; i < 16; ++i) T[i] = cur[i];
            return APD_OK;
        }
        if (!apd_reg_solve(m, with_scale, S)) break;
        apd_reg_mul4(S, cur, cur);
        prev = *info;
        ++it;
    }
    for (int i = 0; i < 16; ++i) T[i] = valid[i];
    return APD_ESTATE;
}

#endif  // APD_REGISTER_H_
