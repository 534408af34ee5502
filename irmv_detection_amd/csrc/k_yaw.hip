// Constrained pose (include/irmv_hip.h, "constrained pose"): the plate's yaw at its known tilt, one 64-lane wavefront per
// detection.  A module of its own, compiled with -ffp-contract=off: every fp64 operation below is the one written, in the
// written order, and irmv_detection_amd/yaw_solve.py follows it operation for operation.  The loop holds +, -, *, / only; the
// square roots of the model (|g|, c) are the host's (engine_yaw.cpp), the one of err is taken once, for the winner.
//
// No LDS: the argmin over the wave is a butterfly of __shfl_xor on (q, lane), after which every lane holds the winner, so
// the next interval is uniform without a broadcast.  fp64 division is the expensive operation here (a correctly rounded
// v_div sequence of ~ 10 instructions): an evaluation has 13 of them (cs, sn, three of the translation, eight residuals)
// among ~ 250 other fp64 operations, and they are the model's, not reciprocals, so that the host can follow them.
#include <hip/hip_runtime.h>

#include "irmv_common.hpp"
#include "pnp_device.hpp"

namespace irmv {

struct YawEval { double R[9]; double t[3]; double cs, sn, q; };

// R(tau), the translation and the cost q of one parameter.  R is row-major model -> camera, columns (n, y, z).
__device__ inline void yaw_eval(const YawRule &r, const double *cX, const double *cY, const double *nxy, double tau, YawEval &e)
{
    const double inf = __builtin_huge_val();
    const double tt = tau * tau;
    const double d = 1.0 + tt;
    const double cs = (1.0 - tt) / d, sn = (2.0 * tau) / d;
    double n[3], y[3];
    for (int i = 0; i < 3; i++) {
        n[i] = r.s * r.u[i] + r.c * (cs * r.h1[i] + sn * r.h2[i]);
        y[i] = cs * r.h2[i] - sn * r.h1[i];
    }
    const double z[3] = {n[1] * y[2] - n[2] * y[1], n[2] * y[0] - n[0] * y[2], n[0] * y[1] - n[1] * y[0]};
    // the solver's canonical frame: columns (Xc, Yc, Zc) = (y_model, z_model, x_model)
    double Rc[9];
    for (int i = 0; i < 3; i++) { Rc[i * 3 + 0] = y[i]; Rc[i * 3 + 1] = z[i]; Rc[i * 3 + 2] = n[i]; }
    for (int i = 0; i < 3; i++) { e.R[i * 3 + 0] = n[i]; e.R[i * 3 + 1] = y[i]; e.R[i * 3 + 2] = z[i]; }
    e.cs = cs; e.sn = sn;
    bool ok = ippe_translation(cX, cY, nxy, Rc, e.t);
    if (!ok) { e.t[0] = e.t[1] = e.t[2] = 0.0; }
    double q = 0.0;
    for (int i = 0; i < 4; i++) {
        const double X = Rc[0] * cX[i] + Rc[1] * cY[i] + e.t[0];
        const double Y = Rc[3] * cX[i] + Rc[4] * cY[i] + e.t[1];
        const double Z = Rc[6] * cX[i] + Rc[7] * cY[i] + e.t[2];
        if (!(Z > 0.0)) ok = false;
        const double ex = X / Z - nxy[2 * i], ey = Y / Z - nxy[2 * i + 1];
        q += ex * ex + ey * ey;
    }
    const double nt = (n[0] * e.t[0] + n[1] * e.t[1]) + n[2] * e.t[2];
    if (!(nt > 0.0)) ok = false;
    e.q = (ok && q < inf) ? q : inf;   // (negated where it matters: a NaN is +inf)
}

// One detection on the whole wave: every lane returns the same record.  pts: LB, LT, RT, RB in source-frame pixels.
__device__ inline DevYaw yaw_solve_wave(const PnpConst &pc, const float *pts, int armor_size, const YawRule &r)
{
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_huge_val();
    DevYaw o{};
    for (int i = 0; i < 8; i++)
        if (!pixel_in_range(pts[i])) return o;           // (uniform: every lane has the same points)
    for (int k = 0; k < kYawRoundsMax; k++) o.lane[k] = -1;
    o.state = -1;
    if (!r.ok || !(r.c > 0.0)) return o;
    const double hy = pc.hy[armor_size & 1], hz = pc.hz[armor_size & 1];
    double nxy[8];
    undistort4(pc, pts, nxy);
    const double cX[4] = {hy, hy, -hy, -hy}, cY[4] = {-hz, hz, hz, -hz};
    double lo = -r.tau_max, hi = r.tau_max, tau = 0.0;
    YawEval e;
    for (int round = 0; round < r.rounds; round++) {
        const double span = hi - lo;
        yaw_eval(r, cX, cY, nxy, lo + (span * (double)lane) / 63.0, e);
        double q = e.q;
        int k = lane;
        for (int m = 1; m < 64; m <<= 1) {               // butterfly: afterwards every lane holds the wave's (q, k)
            const double oq = __shfl_xor(q, m);
            const int ok = __shfl_xor(k, m);
            if (oq < q || (oq == q && ok < k)) { q = oq; k = ok; }
        }
        if (round == 0 && !(q < inf)) return o;          // no admissible lane
        o.lane[round] = k;
        tau = lo + (span * (double)k) / 63.0;
        const double step = span / 63.0;
        lo = fmax(tau - step, -r.tau_max);
        hi = fmin(tau + step, r.tau_max);
    }
    yaw_eval(r, cX, cY, nxy, tau, e);                    // the winner's, on every lane: the bits its lane had
    if (!(e.q < inf)) return o;
    rot_to_rvec(e.R, o.rvec);
    rot_to_quat(e.R, o.quat);
    o.tvec[0] = e.t[0]; o.tvec[1] = e.t[1]; o.tvec[2] = e.t[2];
    o.tau = tau; o.cs = e.cs; o.sn = e.sn;
    o.err = sqrt(e.q / 8.0);
    if (!pose_finite(o.rvec, o.tvec)) {
        DevYaw f{};
        for (int k = 0; k < kYawRoundsMax; k++) f.lane[k] = o.lane[k];
        f.state = -1;
        return f;
    }
    o.state = 1;
    return o;
}

// kYawPerBlock detections per workgroup, one per wave; grid (ceil(max_det / kYawPerBlock), batch)
__global__ __launch_bounds__(kYawThreads) void yaw_solve_kernel(YawArgs a)
{
    const YawTable &tb = *a.table;
    if (!tb.enable) return;
    const int b = blockIdx.y, j = blockIdx.x * kYawPerBlock + (threadIdx.x >> 6);
    const int ndet = min(a.num_dets[b * a.num_dets_stride], a.max_det);
    if (j >= ndet) return;
    const DevDet &d = a.dets[(size_t)b * a.max_det + j];
    DevYaw o{};
    if (d.pnp_ok != 0 && d.armor_valid == 1) {
        float pts[8];
        for (int i = 0; i < 8; i++) pts[i] = d.kpts[i];
        const YawBasis &bs = a.basis[a.first + b];
        // a class outside the table (none the NMS writes) has no tilt: refused, not wrapped onto another class's
        const bool cls_ok = (unsigned)d.cls < (unsigned)kMaxClasses;
        const int cls = d.cls & (kMaxClasses - 1);
        YawRule r;
        for (int i = 0; i < 3; i++) { r.u[i] = bs.u[i]; r.h1[i] = bs.h1[i]; r.h2[i] = bs.h2[i]; }
        r.s = tb.s[cls]; r.c = tb.c[cls]; r.tau_max = tb.tau_max;
        r.rounds = min(max(tb.rounds, 1), kYawRoundsMax); r.ok = (bs.ok && cls_ok) ? 1 : 0;
        o = yaw_solve_wave(a.pnp[(size_t)(a.first + b) * a.pnp_stride], pts, d.armor_size, r);
    }
    if ((threadIdx.x & 63) == 0) a.out[(size_t)b * a.max_det + j] = o;
}

__global__ __launch_bounds__(kYawThreads) void yaw_points_kernel(PnpConst c, const float *pts, int n, int armor_size, YawRule r, DevYaw *out)
{
    const int j = blockIdx.x * kYawPerBlock + (threadIdx.x >> 6);
    if (j >= n) return;
    float p[8];
    for (int i = 0; i < 8; i++) p[i] = pts[(size_t)j * 8 + i];
    const DevYaw o = yaw_solve_wave(c, p, armor_size, r);
    if ((threadIdx.x & 63) == 0) out[j] = o;
}

void launch_yaw_solve(const YawArgs &a, int batch, hipStream_t s)
{
    if (a.max_det <= 0 || batch <= 0) return;
    hipLaunchKernelGGL(yaw_solve_kernel, dim3((a.max_det + kYawPerBlock - 1) / kYawPerBlock, batch), dim3(kYawThreads), 0, s, a);
}

void launch_yaw_points(const PnpConst &c, const float *pts, int n, int armor_size, const YawRule &rule, DevYaw *out, hipStream_t s)
{
    if (n <= 0) return;
    YawRule r = rule;
    r.rounds = r.rounds < 1 ? 1 : (r.rounds > kYawRoundsMax ? kYawRoundsMax : r.rounds);
    hipLaunchKernelGGL(yaw_points_kernel, dim3((n + kYawPerBlock - 1) / kYawPerBlock), dim3(kYawThreads), 0, s, c, pts, n, armor_size, r, out);
}

}  // namespace irmv
