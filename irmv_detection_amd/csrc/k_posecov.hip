// Pose uncertainty (include/irmv_hip.h, "pose uncertainty"): the first-order covariance of a record's IPPE pose (6 x 6) and
// of its constrained pose (4 x 4), one 64-lane wavefront per detection.  A module of its own, compiled with
// -ffp-contract=off: every fp64 operation below is the one written, in the written order, and
// irmv_detection_amd/pose_cov.py follows it operation for operation.  +, -, *, /, sqrt and rint only: the rotation of a
// rotation vector takes sin and cos from two stated series (sin_vers), because no libm is the same on host and device.
//
// The residual is a PIXEL residual that ignores the distortion's own Jacobian: r = (projected - undistorted) * f / sigma_px
// on normalised coordinates.
//
// Lane map.  Lanes 0 .. 47 each own one entry of the 8 x 6 Jacobian (row = lane / 6, column = lane % 6), lanes 0 .. 31 one of
// the yaw block's 8 x 4 (row = lane / 4, column = lane % 4); lanes 0 .. 20 one entry of A = J^T J, lanes 0 .. 9 one of A_yaw;
// lane c solves column c of the inverse.  Entries cross lanes by __shfl (ds_bpermute: no LDS allocation, no ordering point
// between a wave's writers and readers): 8 x 2 operands per entry of A and of A_yaw, 21 + 10 broadcasts of each and of their
// inverses, 8 + 8 residuals -- 114 doubles, 228 ds_bpermute a wave.  The Cholesky factor is computed on every lane from the broadcast A (it is the same
// 21 numbers everywhere), in the reference's order.  fp64 issues at a quarter of the fp32 rate and a division is a ~ 10
// instruction sequence: the 36 + 16 divisions of the two inverses run on six and four lanes at once instead of one after
// another, which is where a serial form would spend its time.
#include <hip/hip_runtime.h>

#include "irmv_common.hpp"
#include "pnp_device.hpp"

namespace irmv {

__device__ inline bool pc_finite(double v) { return fabs(v) < __builtin_huge_val(); }   // (a NaN fails too)
__device__ inline bool pc_in_range(double v) { return fabs(v) < 1e300; }

// (sin th, 1 - cos th) of th >= 0: the angle reduced by the nearest multiple of 2 pi, then the series of sin(a) / a and
// (1 - cos a) / a^2 in a^2 as nested divisions by the integers (2k)(2k + 1) and (2k + 1)(2k + 2)
__device__ inline void sin_vers(double th, double &sn, double &vc)
{
    const double two_pi = 6.283185307179586;
    const double k = rint(th / two_pi);
    const double a = th - k * two_pi;
    const double x = a * a;
    double s = 1.0, c = 1.0;
#pragma unroll
    for (int j = kPoseCovSeriesTerms - 1; j > 0; j--) {
        s = 1.0 - (x / (double)((2 * j) * (2 * j + 1))) * s;
        c = 1.0 - (x / (double)((2 * j + 1) * (2 * j + 2))) * c;
    }
    sn = a * s;
    vc = x * (0.5 * c);
}

// rvec -> R, row-major (model -> camera)
__device__ inline void posecov_rodrigues(const double *r, double *R)
{
    const double th = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    double sn, vc;
    sin_vers(th, sn, vc);
    const double den = th > 0.0 ? th : 1.0;
    const double n0 = r[0] / den, n1 = r[1] / den, n2 = r[2] / den;
    const double d = 1.0 - vc;
    R[0] = d + vc * (n0 * n0);         R[1] = vc * (n0 * n1) - sn * n2;   R[2] = vc * (n0 * n2) + sn * n1;
    R[3] = vc * (n0 * n1) + sn * n2;   R[4] = d + vc * (n1 * n1);         R[5] = vc * (n1 * n2) - sn * n0;
    R[6] = vc * (n0 * n2) - sn * n1;   R[7] = vc * (n1 * n2) + sn * n0;   R[8] = d + vc * (n2 * n2);
}

// The lane's row of the 8 x 6 Jacobian and with it its corner (LB, LT, RT, RB); lanes 48 .. 63 repeat row 7
__device__ inline int posecov_row() { return min((int)(threadIdx.x & 63) / 6, 7); }

// One point of undistort4 (pnp_device.hpp): the same operations on the same values
__device__ inline void posecov_undistort1(const PnpConst &c, float px, float py, double &nx, double &ny)
{
    const double x0 = ((double)px - c.cx) / c.fx, y0 = ((double)py - c.cy) / c.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        const double dx = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
        const double dy = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    nx = x;
    ny = y;
}

// This lane's entry (row, col) of the 8 x 6 Jacobian of the pose (rvec, t) and its row's residual; (nx, ny): the lane's
// undistorted corner.  false on a lane whose corner has depth <= 0 (or NaN).
__device__ inline bool posecov_entry(const double *rvec, const double *t, double nx, double ny, double hy, double hz, double fx, double fy,
                                     double sigma, double &entry, double &res)
{
    const int row = posecov_row(), col = (int)(threadIdx.x & 63) % 6, i = row >> 1;
    double R[9];
    posecov_rodrigues(rvec, R);
    const double cX = i < 2 ? hy : -hy, cY = (i == 1 || i == 2) ? hz : -hz;
    const double a0 = R[1] * cX + R[2] * cY, a1 = R[4] * cX + R[5] * cY, a2 = R[7] * cX + R[8] * cY;
    const double X = a0 + t[0], Y = a1 + t[1], Z = a2 + t[2];
    const bool ok = Z > 0.0;
    const double x = X / Z, y = Y / Z;
    const double sx = fx / sigma, sy = fy / sigma;
    double g0, g1, g2;
    if (row & 1) {
        res = ((y - ny) * fy) / sigma;
        const double gy1 = sy / Z;
        g0 = 0.0; g1 = gy1; g2 = -(y * gy1);
    } else {
        res = ((x - nx) * fx) / sigma;
        const double gx0 = sx / Z;
        g0 = gx0; g1 = 0.0; g2 = -(x * gx0);
    }
    const double j0 = g2 * a1 - g1 * a2, j1 = g0 * a2 - g2 * a0, j2 = g1 * a0 - g0 * a1;
    entry = col == 0 ? j0 : col == 1 ? j1 : col == 2 ? j2 : col == 3 ? g0 : col == 4 ? g1 : g2;
    return ok;
}

// The eight squared residuals, summed in ascending row order; row r's residual sits on lane r * 6
__device__ inline double posecov_chi2(double res)
{
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const double v = __shfl(res, r * 6);
        s = s + v * v;
    }
    return s;
}

// A = J^T J of an 8 x N Jacobian whose entry (r, c) sits on lane r * N + c, on every lane: the upper triangle row-major, each
// entry summed over the rows in ascending order (on the lane that owns it, then broadcast)
template <int N> __device__ inline void posecov_normal(double entry, double *A)
{
    const int lane = threadIdx.x & 63;
    int ii = 0, jj = 0, idx = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++, idx++)
            if (idx == lane) { ii = i; jj = j; }
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 8; r++) acc = acc + __shfl(entry, r * N + ii) * __shfl(entry, r * N + jj);
#pragma unroll
    for (int k = 0; k < N * (N + 1) / 2; k++) A[k] = __shfl(acc, k);
}

// A (upper triangle, row-major; the same on every lane) -> the upper triangle of its inverse on every lane: Cholesky
// A = L L^T column by column, then column c of the inverse on lane c by L y = e_c and L^T x = y; entry (i, j), i <= j, is
// entry i of column j.  false where a pivot p has !(p > 0).
template <int N> __device__ inline bool posecov_inverse(const double *A, double *inv)
{
    const int c = threadIdx.x & 63;
    double L[N][N];
    bool ok = true;
    int at = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        // row j of the upper triangle starts at `at`: A(j, i) = A[at + i - j]
        double p = A[at];
#pragma unroll
        for (int k = 0; k < j; k++) p = p - L[j][k] * L[j][k];
        if (!(p > 0.0)) { ok = false; p = 1.0; }   // (uniform; carried as a flag so that the shuffles below stay converged)
        L[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = A[at + i - j];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
        at += N - j;
    }
    double y[N], x[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        double s = k == c ? 1.0 : 0.0;
#pragma unroll
        for (int m = 0; m < k; m++) s = s - L[k][m] * y[m];
        y[k] = s / L[k][k];
    }
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {
        double s = y[k];
#pragma unroll
        for (int m = k + 1; m < N; m++) s = s - L[m][k] * x[m];
        x[k] = s / L[k][k];
    }
    int o = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++) inv[o++] = __shfl(x[i], j);
    return ok;
}

// One detection on the whole wave: every lane returns the same record.  pts: LB, LT, RT, RB in source-frame pixels, in
// memory: a lane reads its own corner, so that no array is indexed by the lane (such an array is put into LDS); (rvec,
// tvec): the pose of the 6 x 6 block; has_yaw: (yrvec, ytvec) is a constrained pose about the unit vector u.
__device__ inline DevPoseCov posecov_wave(const PnpConst &pc, const float *pts, int armor_size, const double *rvec, const double *tvec,
                                         double sigma, bool has_yaw, const double *yrvec, const double *ytvec, const double *u)
{
    DevPoseCov o{};
    o.state = -1;
    const int pt = posecov_row() >> 1;
    const float px = pts[2 * pt], py = pts[2 * pt + 1];
    if (!__all(pixel_in_range(px) && pixel_in_range(py))) return o;   // (the wave's lanes cover all four corners)
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (!pc_in_range(rvec[i]) || !pc_in_range(tvec[i])) return o;
    const double hy = pc.hy[armor_size & 1], hz = pc.hz[armor_size & 1];
    double nx, ny;
    posecov_undistort1(pc, px, py, nx, ny);
    double entry, res;
    const bool zok = posecov_entry(rvec, tvec, nx, ny, hy, hz, pc.fx, pc.fy, sigma, entry, res);
    if (!__all(zok)) return o;
    double cov[kPoseCovN];
    {
        double A[kPoseCovN];
        posecov_normal<6>(entry, A);
        if (!posecov_inverse<6>(A, cov)) return o;
    }
    const double chi2 = posecov_chi2(res);
    const double ln = sqrt((tvec[0] * tvec[0] + tvec[1] * tvec[1]) + tvec[2] * tvec[2]);
    const double d[3] = {tvec[0] / ln, tvec[1] / ln, tvec[2] / ln};
    // Sigma_tautau: rows / columns 3 .. 5 of the upper triangle (15, 16, 17 / 18, 19 / 20)
    const double S[3][3] = {{cov[15], cov[16], cov[17]}, {cov[16], cov[18], cov[19]}, {cov[17], cov[19], cov[20]}};
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) q = q + d[i] * ((S[i][0] * d[0] + S[i][1] * d[1]) + S[i][2] * d[2]);
    const double sigma_range = sqrt(q);
    bool fin = pc_finite(chi2) && pc_finite(sigma_range);
#pragma unroll
    for (int k = 0; k < kPoseCovN; k++) fin = fin && pc_finite(cov[k]);
    if (!fin) return o;
#pragma unroll
    for (int k = 0; k < kPoseCovN; k++) o.cov[k] = cov[k];
    o.chi2 = chi2; o.sigma_range = sigma_range;
    o.state = 1;
    if (!has_yaw) return o;
    o.yaw_state = -1;
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (!pc_in_range(yrvec[i]) || !pc_in_range(ytvec[i]) || !pc_in_range(u[i])) return o;
    const bool yzok = posecov_entry(yrvec, ytvec, nx, ny, hy, hz, pc.fx, pc.fy, sigma, entry, res);
    if (!__all(yzok)) return o;
    // the yaw block's entry (row, c) on lane row * 4 + c: c == 0 the rotation block applied to u, else the translation column
    const int lane = threadIdx.x & 63, yrow = min(lane >> 2, 7), yc = lane & 3;
    const double w0 = __shfl(entry, yrow * 6), w1 = __shfl(entry, yrow * 6 + 1), w2 = __shfl(entry, yrow * 6 + 2);
    const double tc = __shfl(entry, yrow * 6 + 2 + max(yc, 1));
    const double yentry = yc == 0 ? (w0 * u[0] + w1 * u[1]) + w2 * u[2] : tc;
    double ycov[kPoseCovYawN];
    {
        double A[kPoseCovYawN];
        posecov_normal<4>(yentry, A);
        if (!posecov_inverse<4>(A, ycov)) return o;
    }
    const double ychi2 = posecov_chi2(res);
    const double sigma_yaw = sqrt(ycov[0]);
    fin = pc_finite(ychi2) && pc_finite(sigma_yaw);
#pragma unroll
    for (int k = 0; k < kPoseCovYawN; k++) fin = fin && pc_finite(ycov[k]);
    if (!fin) return o;
#pragma unroll
    for (int k = 0; k < kPoseCovYawN; k++) o.yaw_cov[k] = ycov[k];
    o.yaw_chi2 = ychi2; o.sigma_yaw = sigma_yaw;
    o.yaw_state = 1;
    return o;
}

// One detection per workgroup of one wave; grid (max_det, batch)
__global__ __launch_bounds__(64) void pose_cov_kernel(PoseCovArgs a)
{
    const PoseCovTable &tb = *a.table;
    if (!tb.enable) return;
    const int b = blockIdx.y, j = blockIdx.x;
    const int ndet = min(a.num_dets[b * a.num_dets_stride], a.max_det);
    if (j >= ndet) return;
    const size_t at = (size_t)b * a.max_det + j;
    const DevDet &d = a.dets[at];
    DevPoseCov o{};
    if (d.pnp_ok != 0 && d.armor_valid == 1) {
        const double rvec[3] = {d.rvec[0], d.rvec[1], d.rvec[2]}, tvec[3] = {d.tvec[0], d.tvec[1], d.tvec[2]};
        double yr[3] = {0.0, 0.0, 0.0}, yt[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        bool has_yaw = false;
        if (a.yaw) {   // (the engine solves yaws: the record the step's yaw launch has just written)
            const DevYaw &y = a.yaw[at];
            has_yaw = y.state == 1;
            if (has_yaw) {
                const YawBasis &bs = a.basis[a.first + b];
                for (int i = 0; i < 3; i++) { yr[i] = y.rvec[i]; yt[i] = y.tvec[i]; u[i] = bs.u[i]; }
            }
        }
        o = posecov_wave(a.pnp[(size_t)(a.first + b) * a.pnp_stride], d.kpts, d.armor_size, rvec, tvec, tb.sigma_px, has_yaw, yr, yt, u);
    }
    if (threadIdx.x == 0) a.out[at] = o;
}

__global__ __launch_bounds__(64) void pose_cov_points_kernel(PnpConst c, const float *pts, const double *poses, int n, int armor_size,
                                                            PoseCovRule r, DevPoseCov *out)
{
    const int j = blockIdx.x;
    if (j >= n) return;
    double rvec[3], tvec[3];
    for (int i = 0; i < 3; i++) { rvec[i] = poses[(size_t)j * 6 + i]; tvec[i] = poses[(size_t)j * 6 + 3 + i]; }
    const DevPoseCov o = posecov_wave(c, pts + (size_t)j * 8, armor_size, rvec, tvec, r.sigma_px, r.has_up != 0, rvec, tvec, r.u);
    if (threadIdx.x == 0) out[j] = o;
}

void launch_pose_cov(const PoseCovArgs &a, int batch, hipStream_t s)
{
    if (a.max_det <= 0 || batch <= 0) return;
    hipLaunchKernelGGL(pose_cov_kernel, dim3(a.max_det, batch), dim3(64), 0, s, a);
}

void launch_pose_cov_points(const PnpConst &c, const float *pts, const double *poses, int n, int armor_size, const PoseCovRule &rule,
                            DevPoseCov *out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(pose_cov_points_kernel, dim3(n), dim3(64), 0, s, c, pts, poses, n, armor_size, rule, out);
}

}  // namespace irmv
