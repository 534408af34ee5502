// Armor tracks: the filter's arithmetic, one copy for the kernel (k_track.hip) and the host helper irmv_track_predict
// (engine_track.cpp).  Both files are compiled with -ffp-contract=off: every fp64 operation below is the one written, in the
// written order, and irmv_detection_amd/tracks.py states the same operations in the same order.  +, -, *, / and comparisons only.
#pragma once
#include "irmv_common.hpp"

namespace irmv {

__host__ __device__ inline bool trk_finite(double v) { return (v < 0.0 ? -v : v) < __builtin_huge_val(); }   // (a NaN fails too)

// tracks.py predict: x, P (row-major 6 x 6, exactly symmetric) moved by dt in place
__host__ __device__ inline void trk_predict(double *x, double *Pm, double dt, double accel_sigma)
{
    const double q = accel_sigma * accel_sigma;
    const double dt2 = dt * dt;
    const double qpp = (q * (dt2 * dt2)) / 4.0;
    const double qpv = (q * (dt2 * dt)) / 2.0;
    const double qvv = q * dt2;
    double P[36], N[36];
#pragma unroll
    for (int i = 0; i < 36; i++) P[i] = Pm[i];
    x[0] = x[0] + dt * x[3];
    x[1] = x[1] + dt * x[4];
    x[2] = x[2] + dt * x[5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double pv = P[i * 6 + j + 3] + dt * P[(i + 3) * 6 + j + 3];
            if (i == j) pv = pv + qpv;
            N[i * 6 + j + 3] = pv;
            N[(j + 3) * 6 + i] = pv;
        }
#pragma unroll
        for (int j = i; j < 3; j++) {
            double pp = (P[i * 6 + j] + dt * (P[(i + 3) * 6 + j] + P[i * 6 + j + 3])) + dt2 * P[(i + 3) * 6 + j + 3];
            double vv = P[(i + 3) * 6 + j + 3];
            if (i == j) {
                pp = pp + qpp;
                vv = vv + qvv;
            }
            N[i * 6 + j] = pp;
            N[j * 6 + i] = pp;
            N[(i + 3) * 6 + j + 3] = vv;
            N[(j + 3) * 6 + i + 3] = vv;
        }
    }
#pragma unroll
    for (int i = 0; i < 36; i++) Pm[i] = N[i];
}

// tracks.py measure's default noise: C = diag((sigma_lat z)^2, (sigma_lat z)^2, (sigma_rng z^2)^2), row-major 3 x 3
__host__ __device__ inline void trk_default_noise(double tz, double sigma_lat, double sigma_rng, double *C)
{
    const double s1 = sigma_lat * tz;
    const double s2 = sigma_rng * (tz * tz);
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = 0.0;
    C[0] = s1 * s1; C[4] = s1 * s1; C[8] = s2 * s2;
}

// tracks.py measure, behind its validity test: z and the upper triangle R6 = (00, 01, 02, 11, 12, 22) of the rotated noise.
// C: the row-major 3 x 3 camera-frame noise.  false: not eligible.
__host__ __device__ inline bool trk_measure(const double *tv, const double *C, const double *Rw, const double *tw, double *z, double *R6)
{
    if (!(trk_finite(tv[0]) && trk_finite(tv[1]) && trk_finite(tv[2])) || !(tv[2] > 0.0)) return false;
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        z[i] = ((Rw[3 * i] * tv[0] + Rw[3 * i + 1] * tv[1]) + Rw[3 * i + 2] * tv[2]) + tw[i];
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = (Rw[3 * i] * C[j] + Rw[3 * i + 1] * C[3 + j]) + Rw[3 * i + 2] * C[6 + j];
    }
    bool ok = trk_finite(z[0]) && trk_finite(z[1]) && trk_finite(z[2]);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            const double r = (M[3 * i] * Rw[3 * j] + M[3 * i + 1] * Rw[3 * j + 1]) + M[3 * i + 2] * Rw[3 * j + 2];
            R6[k++] = r;
            ok = ok && trk_finite(r) && (i != j || r > 0.0);
        }
    return ok;
}

// tracks.py innovation: y and the upper triangle Si6 of S^-1; false where det S is not finite and positive
__host__ __device__ inline bool trk_innovation(const double *x, const double *P, const double *z, const double *R6, double *y, double *Si6)
{
    y[0] = z[0] - x[0]; y[1] = z[1] - x[1]; y[2] = z[2] - x[2];
    const double s00 = P[0] + R6[0], s01 = P[1] + R6[1], s02 = P[2] + R6[2];
    const double s10 = P[6] + R6[1], s11 = P[7] + R6[3], s12 = P[8] + R6[4];
    const double s20 = P[12] + R6[2], s21 = P[13] + R6[4], s22 = P[14] + R6[5];
    const double c00 = s11 * s22 - s12 * s21;
    const double c01 = s12 * s20 - s10 * s22;
    const double c02 = s10 * s21 - s11 * s20;
    const double c11 = s00 * s22 - s02 * s20;
    const double c12 = s01 * s20 - s00 * s21;
    const double c22 = s00 * s11 - s01 * s10;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    if (!(det > 0.0 && det < __builtin_huge_val())) return false;
    Si6[0] = c00 / det; Si6[1] = c01 / det; Si6[2] = c02 / det;
    Si6[3] = c11 / det; Si6[4] = c12 / det; Si6[5] = c22 / det;
    return true;
}

// tracks.py distance2
__host__ __device__ inline double trk_distance2(const double *y, const double *Si6)
{
    const double w0 = (Si6[0] * y[0] + Si6[1] * y[1]) + Si6[2] * y[2];
    const double w1 = (Si6[1] * y[0] + Si6[3] * y[1]) + Si6[4] * y[2];
    const double w2 = (Si6[2] * y[0] + Si6[4] * y[1]) + Si6[5] * y[2];
    return (y[0] * w0 + y[1] * w1) + y[2] * w2;
}

// tracks.py kalman_update, in place
__host__ __device__ inline void trk_update(double *x, double *Pm, const double *y, const double *Si6)
{
    const double Si[9] = {Si6[0], Si6[1], Si6[2], Si6[1], Si6[3], Si6[4], Si6[2], Si6[4], Si6[5]};
    double P[36], K[18];
#pragma unroll
    for (int i = 0; i < 36; i++) P[i] = Pm[i];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) K[i * 3 + j] = (P[i * 6] * Si[j] + P[i * 6 + 1] * Si[3 + j]) + P[i * 6 + 2] * Si[6 + j];
        x[i] = x[i] + ((K[i * 3] * y[0] + K[i * 3 + 1] * y[1]) + K[i * 3 + 2] * y[2]);
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            const double v = P[i * 6 + j] - ((K[i * 3] * P[j] + K[i * 3 + 1] * P[6 + j]) + K[i * 3 + 2] * P[12 + j]);
            Pm[i * 6 + j] = v;
            Pm[j * 6 + i] = v;
        }
}

}   // namespace irmv
