// Plate patches (include/irmv_hip.h, "plate patches"): each armor's rectified 20 x 28 gray number image, its Otsu threshold
// and the colour vote of its two light bars, one 64-lane wavefront per detection.  A module of its own, compiled with
// -ffp-contract=off: every fp64 operation below is the one written, in the written order, and
// irmv_detection_amd/patches.py follows it operation for operation; everything behind the quantisation is integer.
//
// A lane owns 32-bit words of the patch -- four neighbouring samples of a row, 140 words, three rounds -- so that every
// store to the record is a whole dword (a zero-copy engine's records are pinned host memory).  The 256-bin histogram of a
// wave is its own 1 KiB of LDS, filled with LDS atomics and read back by the same wave: wave-scope fences order it, and NO
// workgroup barrier exists in this file -- waves leave early (past num_dets, enable = 0) and the others must not wait.
#include <hip/hip_runtime.h>

#include "irmv_common.hpp"

namespace irmv {

__device__ inline void patch_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct PatchFrame { const uint8_t *px; int W, H, rot; };

// The texel of view coordinates (ix, iy), or nullptr outside the frame: no address outside [0, W) x [0, H) is ever formed
__device__ inline const uint8_t *patch_texel(const PatchFrame &f, int ix, int iy)
{
    if ((unsigned)ix >= (unsigned)f.W || (unsigned)iy >= (unsigned)f.H) return nullptr;
    const int sx = f.rot ? f.W - 1 - ix : ix, sy = f.rot ? f.H - 1 - iy : iy;
    return f.px + ((size_t)sy * f.W + sx) * 3;
}

__device__ inline int patch_gray(const PatchFrame &f, int ix, int iy)
{
    const uint8_t *p = patch_texel(f, ix, iy);
    return p ? (p[0] * 3735 + p[1] * 19235 + p[2] * 9798 + (1 << 14)) >> 15 : 0;
}

// Heckbert's square-to-quad of LB, LT, RT, RB: co = a b c d e f g h.  false: the record has no patch.
__device__ inline bool patch_coefficients(const float *k, double *co)
{
    for (int i = 0; i < 8; i++)
        if (!__builtin_isfinite(k[i])) return false;
    const double x0 = k[2], y0 = k[3], x1 = k[4], y1 = k[5], x2 = k[6], y2 = k[7], x3 = k[0], y3 = k[1];
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = ((x0 - x1) + x2) - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = ((y0 - y1) + y2) - y3;
    const double den = dx1 * dy2 - dx2 * dy1;
    if (den == 0.0) return false;
    const double g = (sx * dy2 - dx2 * sy) / den;
    const double h = (dx1 * sy - sx * dy1) / den;
    co[0] = (x1 - x0) + g * x1; co[1] = (x3 - x0) + h * x3; co[2] = x0;
    co[3] = (y1 - y0) + g * y1; co[4] = (y3 - y0) + h * y3; co[5] = y0;
    co[6] = g; co[7] = h;
    for (int i = 0; i < 8; i++)
        if (!__builtin_isfinite(co[i])) return false;
    return true;
}

struct PatchXY { double x, y, w; };
__device__ inline PatchXY patch_map(const double *co, double s, double t)
{
    PatchXY p;
    p.w = (co[6] * s + co[7] * t) + 1.0;
    p.x = ((co[0] * s + co[1] * t) + co[2]) / p.w;
    p.y = ((co[3] * s + co[4] * t) + co[5]) / p.w;
    return p;
}

__device__ inline bool patch_near(const PatchFrame &f, double x, double y)
{
    return x >= -1.0 && x <= (double)f.W && y >= -1.0 && y <= (double)f.H;   // (a NaN fails)
}

__device__ inline int patch_wave_sum(int v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// One quad on the whole wave: every lane has the same k and size; hist: the wave's 256 words of LDS; o: the record.
__device__ inline void patch_wave(const PatchFrame &f, bool armor, const float *k, int armor_size, const PatchTable &tb, uint32_t *hist, DevPatch *o)
{
    const int lane = threadIdx.x & 63;
    uint32_t *words = reinterpret_cast<uint32_t *>(o);
    constexpr int kRecWords = (int)(sizeof(DevPatch) / 4);
    double co[8];
    bool ok = armor && patch_coefficients(k, co);           // (uniform)
    uint32_t word[3] = {0u, 0u, 0u};
    int outside = 0;
    if (ok) {
        const int span = tb.span[armor_size & 1], off = (span - kPatchW) / 2;
        bool bad = false;
        for (int r = 0; r < 3; r++) {
            const int wi = lane + 64 * r;
            if (wi >= kPatchWords) break;
            const int j = wi / (kPatchW / 4), i0 = (wi % (kPatchW / 4)) * 4;
            const double t = (double)(j - tb.top) / (double)tb.light_rows;
            for (int q = 0; q < 4; q++) {
                const double s = (double)(i0 + q + off) / (double)(span - 1);
                const PatchXY p = patch_map(co, s, t);
                if (!(p.w > 0.0)) bad = true;
                if (!(p.x >= 0.0 && p.x <= (double)(f.W - 1) && p.y >= 0.0 && p.y <= (double)(f.H - 1))) outside++;
                int v = 0;
                if (patch_near(f, p.x, p.y)) {
                    const int X = (int)floor(32.0 * p.x + 0.5), Y = (int)floor(32.0 * p.y + 0.5);
                    const int ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31;
                    const int g00 = patch_gray(f, ix, iy), g10 = patch_gray(f, ix + 1, iy);
                    const int g01 = patch_gray(f, ix, iy + 1), g11 = patch_gray(f, ix + 1, iy + 1);
                    v = (g00 * (32 - fx) * (32 - fy) + g10 * fx * (32 - fy) + g01 * (32 - fx) * fy + g11 * fx * fy + 512) >> 10;
                }
                word[r] |= (uint32_t)v << (8 * q);
            }
        }
        if (__any(bad)) ok = false;                          // a horizon inside the patch
    }
    if (!ok) {                                               // no patch: all 592 bytes zero
        for (int wi = lane; wi < kRecWords; wi += 64) words[wi] = 0u;
        return;
    }
    // Otsu: the wave's histogram, then four levels a lane
    for (int q = 0; q < 4; q++) hist[lane * 4 + q] = 0u;
    patch_wave_sync();
    for (int r = 0; r < 3; r++)
        if (lane + 64 * r < kPatchWords)
            for (int q = 0; q < 4; q++) atomicAdd(&hist[(word[r] >> (8 * q)) & 255u], 1u);
    patch_wave_sync();
    int hq[4], cnt = 0, sm = 0;
    for (int q = 0; q < 4; q++) { hq[q] = (int)hist[lane * 4 + q]; cnt += hq[q]; sm += hq[q] * (lane * 4 + q); }
    int icnt = cnt, ism = sm;                                // inclusive prefix over the lanes
    for (int m = 1; m < 64; m <<= 1) {
        const int c = __shfl_up(icnt, m), s2 = __shfl_up(ism, m);
        if (lane >= m) { icnt += c; ism += s2; }
    }
    const long long N = kPatchN, S = __shfl(ism, 63);
    long long w0 = icnt - cnt, m0 = ism - sm;
    double bq = -1.0;
    int bk = lane * 4;
    for (int q = 0; q < 4; q++) {
        w0 += hq[q]; m0 += (long long)hq[q] * (lane * 4 + q);
        const long long w1 = N - w0;
        double qk = -1.0;
        if (w0 > 0 && w1 > 0) {
            const long long A = m0 * N - S * w0;
            qk = (double)(A * A) / (double)(w0 * w1);
        }
        if (qk > bq) { bq = qk; bk = lane * 4 + q; }
    }
    for (int m = 1; m < 64; m <<= 1) {                       // butterfly: the smallest k of maximal q, on every lane
        const double oq = __shfl_xor(bq, m);
        const int okk = __shfl_xor(bk, m);
        if (oq > bq || (oq == bq && okk < bk)) { bq = oq; bk = okk; }
    }
    const int otsu = bq < 0.0 ? (int)(S / N) : bk;           // one gray level: that level
    outside = patch_wave_sum(outside);
    // the bars' colour vote: 2 (light_rows + 1) <= 58 points, one a lane
    int c0 = 0, c2 = 0;
    const int per = tb.light_rows + 1;
    if (lane < 2 * per) {
        const int side = lane / per, r = lane % per;
        const PatchXY p = patch_map(co, side ? 1.0 : 0.0, (double)r / (double)tb.light_rows);
        if (patch_near(f, p.x, p.y)) {
            const int X = (int)floor(32.0 * p.x + 0.5), Y = (int)floor(32.0 * p.y + 0.5);
            const uint8_t *px = patch_texel(f, (X + 16) >> 5, (Y + 16) >> 5);
            if (px) { c0 = px[0]; c2 = px[2]; }
        }
    }
    c0 = patch_wave_sum(c0);
    c2 = patch_wave_sum(c2);
    for (int r = 0; r < 3; r++)
        if (lane + 64 * r < kPatchWords) words[lane + 64 * r] = word[r];
    if (lane < 8) {
        const uint32_t tail[8] = {1u, (uint32_t)otsu, (uint32_t)outside, (uint32_t)armor_size, (uint32_t)c0, (uint32_t)c2, (uint32_t)S, 0u};
        uint32_t v = 0u;
        for (int q = 0; q < 8; q++) v = lane == q ? tail[q] : v;
        words[kPatchWords + lane] = v;
    }
}

// kPatchPerBlock detections per workgroup, one per wave; grid (ceil(max_det / kPatchPerBlock), batch)
__global__ __launch_bounds__(kPatchThreads) void patch_step_kernel(PatchArgs a)
{
    __shared__ uint32_t s_hist[kPatchPerBlock][256];
    const PatchTable &tb = *a.table;
    if (!tb.enable) return;
    const int b = blockIdx.y, wave = threadIdx.x >> 6, j = blockIdx.x * kPatchPerBlock + wave;
    const int ndet = min(a.num_dets[b * a.num_dets_stride], a.max_det);
    if (j >= ndet) return;
    const DevDet &d = a.dets[(size_t)b * a.max_det + j];
    float k[8];
    for (int i = 0; i < 8; i++) k[i] = d.kpts[i];
    const PatchFrame f{a.frames + (size_t)b * a.frame_bytes, a.W, a.H, a.rotate180};
    patch_wave(f, d.armor_valid == 1, k, d.armor_size, tb, s_hist[wave], a.out + (size_t)b * a.max_det + j);
}

__global__ __launch_bounds__(kPatchThreads) void patch_points_kernel(PatchArgs a, const float *kpts, const int32_t *sizes, int n)
{
    __shared__ uint32_t s_hist[kPatchPerBlock][256];
    const int wave = threadIdx.x >> 6, j = blockIdx.x * kPatchPerBlock + wave;
    if (j >= n) return;
    float k[8];
    for (int i = 0; i < 8; i++) k[i] = kpts[(size_t)j * 8 + i];
    const PatchFrame f{a.frames, a.W, a.H, a.rotate180};
    patch_wave(f, true, k, sizes[j], *a.table, s_hist[wave], a.out + j);
}

void launch_patch_step(const PatchArgs &a, int batch, hipStream_t s)
{
    if (a.max_det <= 0 || batch <= 0) return;
    hipLaunchKernelGGL(patch_step_kernel, dim3((a.max_det + kPatchPerBlock - 1) / kPatchPerBlock, batch), dim3(kPatchThreads), 0, s, a);
}

void launch_patch_points(const PatchArgs &a, const float *kpts, const int32_t *sizes, int n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(patch_points_kernel, dim3((n + kPatchPerBlock - 1) / kPatchPerBlock), dim3(kPatchThreads), 0, s, a, kpts, sizes, n);
}

}  // namespace irmv
