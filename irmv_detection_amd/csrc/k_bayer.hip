// Raw Bayer camera frames -> the engine's HWC source frames, for gfx950.
//
// A camera's native 8-bit CFA frame is a third of the bytes of its RGB rendering: the producer hands the sensor buffer over
// as it is, it crosses PCIe at W*H bytes, and this kernel rebuilds the R, G, B frame in HBM that every later kernel
// (front_fused / preprocess, rotate180, the light extraction) reads unchanged.
//
// Algorithm (bit-exact with irmv_detection_amd/bayer.py): integer bilinear interpolation, round half up, reflect-101
// borders (-1 -> 1, W -> W-2: the CFA phase is kept, so the interior formulas hold at the edges), then per-channel Q8
// gains min(255, (v g + 128) >> 8).
//
// Two more kernels end in a table look-up T[c][v] instead of the gain arithmetic (T: [3][256] bytes, the gains and a tone LUT
// folded on the host, irmv_engine_set_bayer_isp; staged in LDS in front of the rows): bayer_demosaic_lut_kernel, the same
// bilinear interpolation, and bayer_demosaic_mhc_kernel, the 5 x 5 Malvar-He-Cutler filters in sixteenths (include/irmv_hip.h,
// IRMV_DEMOSAIC_MHC), with two halo rows and columns, reflect-101 at radius 2.  An engine that never sets a table and asks
// for bilinear launches bayer_demosaic_kernel alone.
//
// Work layout: one workgroup per band of kBayerBandRows output rows of one frame.  The band and its halo rows are one
// contiguous byte range of the raw frame; it is staged in LDS with 16-byte loads (bytes at the unaligned ends), at the
// same offset modulo 16 it has in memory, so every aligned global chunk lands in an aligned LDS slot.  Each lane then
// produces a run of 16 pixels of one row (48 output bytes, three 16-byte stores where the destination is aligned).
// Memory-bound: per 1280 x 1024 frame 1.31 MB in (plus the halo rows, mostly L2 hits) and 3.93 MB out.
#include "irmv_common.hpp"

namespace irmv {

constexpr int kRun = 16;   // pixels per lane task

__device__ __forceinline__ uint32_t apply_gain(uint32_t v, uint32_t g)
{
    const uint32_t r = (v * g + 128u) >> 8;
    return r < 255u ? r : 255u;
}

// One band: stage, then demosaic.  `lds` holds (band rows + 2) * W + 16 bytes.
__device__ __forceinline__ void demosaic_band(const BayerArgs &a, const uint8_t *raw, uint8_t *dst, int band, uint8_t *lds)
{
    const int W = a.W, H = a.H;
    const int y0 = band * kBayerBandRows, y1 = min(y0 + kBayerBandRows, H);
    const int ylo = max(y0 - 1, 0), yhi = min(y1 + 1, H);   // staged rows [ylo, yhi): reflect-101 maps rows -1 and H into them
    const uint8_t *src = raw + (size_t)ylo * W;
    const int nbytes = (yhi - ylo) * W;
    const int mis = (int)((uintptr_t)src & 15);               // LDS index of source byte k: k + mis
    const int head = min((16 - mis) & 15, nbytes);
    const int n16 = (nbytes - head) >> 4;
    const int tail0 = head + (n16 << 4);
    for (int k = threadIdx.x; k < head; k += blockDim.x) lds[mis + k] = src[k];
    for (int i0 = threadIdx.x; i0 < n16; i0 += 4 * blockDim.x) {   // four loads in flight per lane before the LDS writes
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n16) v[u] = *reinterpret_cast<const u32x4 *>(src + head + 16 * i);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n16) *reinterpret_cast<u32x4 *>(lds + mis + head + 16 * i) = v[u];
        }
    }
    for (int k = tail0 + (int)threadIdx.x; k < nbytes; k += blockDim.x) lds[mis + k] = src[k];
    __syncthreads();

    const int nrun = (W + kRun - 1) / kRun;
    const int tasks = (y1 - y0) * nrun;
    // fast LDS reads when every staged row starts on a 16-byte boundary (W % 16 == 0 and an aligned band start)
    const bool aligned = ((W | mis) & 15) == 0;
    for (int t = threadIdx.x; t < tasks; t += blockDim.x) {
        const int y = y0 + t / nrun, x0 = (t % nrun) * kRun;
        const int yn = y == 0 ? 1 : y - 1, ys = y == H - 1 ? H - 2 : y + 1;
        const int rows[3] = {yn, y, ys};
        // p[k][j] = raw(row k, column x0 - 1 + j), j = 0..17, reflect-101 at the frame's left and right edges
        uint32_t p[3][kRun + 2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint8_t *r = lds + mis + (rows[k] - ylo) * W;
            const int xl = x0 == 0 ? 1 : x0 - 1;
            p[k][0] = r[xl];
            if (aligned && x0 + kRun <= W) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(r + x0);
#pragma unroll
                for (int j = 0; j < kRun; j++) p[k][j + 1] = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
            } else {
#pragma unroll
                for (int j = 0; j < kRun; j++) {
                    const int x = x0 + j;
                    p[k][j + 1] = r[x < W ? x : (x == W ? W - 2 : W - 1)];   // (columns past W belong to pixels that are not stored)
                }
            }
            const int xr = x0 + kRun;
            p[k][kRun + 1] = r[xr < W ? xr : (xr == W ? W - 2 : W - 1)];
        }
        const bool r_row = (y & 1) == a.ry;
        uint32_t out[3 * kRun];
#pragma unroll
        for (int j = 0; j < kRun; j++) {
            const uint32_t c = p[1][j + 1];
            const uint32_t cross = (p[0][j + 1] + p[2][j + 1] + p[1][j] + p[1][j + 2] + 2u) >> 2;
            const uint32_t diag = (p[0][j] + p[0][j + 2] + p[2][j] + p[2][j + 2] + 2u) >> 2;
            const uint32_t horiz = (p[1][j] + p[1][j + 2] + 1u) >> 1;
            const uint32_t vert = (p[0][j + 1] + p[2][j + 1] + 1u) >> 1;
            const bool r_col = (j & 1) == a.rx;   // (x0 is even: column parity = j & 1)
            uint32_t R, G, B;
            if (r_row == r_col) {                 // an R or a B site
                G = cross;
                R = r_row ? c : diag;
                B = r_row ? diag : c;
            } else {                              // a G site: its own row's colour from W / E, the other from N / S
                G = c;
                R = r_row ? horiz : vert;
                B = r_row ? vert : horiz;
            }
            out[3 * j + 0] = apply_gain(R, a.gain[0]);
            out[3 * j + 1] = apply_gain(G, a.gain[1]);
            out[3 * j + 2] = apply_gain(B, a.gain[2]);
        }
        uint8_t *d = dst + ((size_t)y * W + x0) * 3;
        if (x0 + kRun <= W && ((uintptr_t)d & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                u32x4 v;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const int b = 16 * q + 4 * w;
                    v[w] = out[b] | (out[b + 1] << 8) | (out[b + 2] << 16) | (out[b + 3] << 24);
                }
                reinterpret_cast<u32x4 *>(d)[q] = v;
            }
        } else {
            const int n = min(kRun, W - x0) * 3;
#pragma unroll
            for (int b = 0; b < 3 * kRun; b++)
                if (b < n) d[b] = (uint8_t)out[b];
        }
    }
}

// grid (bands, frames)
__global__ __launch_bounds__(256) void bayer_demosaic_kernel(BayerArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.y;
    demosaic_band(a, a.raw + (size_t)b * a.raw_slot_bytes, a.dst + (size_t)b * a.dst_slot_bytes, blockIdx.x, lds);
}

// (The helpers below serve the table forms; bayer_demosaic_kernel above stays as it was compiled before they existed.)
// Stage the nbytes at src in LDS at the offset modulo 16 they have in memory (LDS index of source byte k: k + the value
// returned): 16-byte loads, bytes at the unaligned ends.  `lds` is 16-byte aligned and holds nbytes + 16.
__device__ __forceinline__ int stage_rows(const uint8_t *src, int nbytes, uint8_t *lds)
{
    const int mis = (int)((uintptr_t)src & 15);
    const int head = min((16 - mis) & 15, nbytes);
    const int n16 = (nbytes - head) >> 4;
    const int tail0 = head + (n16 << 4);
    for (int k = threadIdx.x; k < head; k += blockDim.x) lds[mis + k] = src[k];
    for (int i0 = threadIdx.x; i0 < n16; i0 += 4 * blockDim.x) {   // four loads in flight per lane before the LDS writes
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n16) v[u] = *reinterpret_cast<const u32x4 *>(src + head + 16 * i);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n16) *reinterpret_cast<u32x4 *>(lds + mis + head + 16 * i) = v[u];
        }
    }
    for (int k = tail0 + (int)threadIdx.x; k < nbytes; k += blockDim.x) lds[mis + k] = src[k];
    return mis;
}

// A lane's 48 output bytes -> dst: three 16-byte stores where the run is whole and the destination aligned.
__device__ __forceinline__ void store_run(uint8_t *d, const uint32_t (&out)[3 * kRun], int x0, int W)
{
    if (x0 + kRun <= W && ((uintptr_t)d & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            u32x4 v;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int b = 16 * q + 4 * w;
                v[w] = out[b] | (out[b + 1] << 8) | (out[b + 2] << 16) | (out[b + 3] << 24);
            }
            reinterpret_cast<u32x4 *>(d)[q] = v;
        }
    } else {
        const int n = min(kRun, W - x0) * 3;
#pragma unroll
        for (int b = 0; b < 3 * kRun; b++)
            if (b < n) d[b] = (uint8_t)out[b];
    }
}

// The table forms.  `lds`: the [3][256] table, then (band rows + 2 R) * W + 16 bytes of rows, R the halo radius (MHC: 2).
template <bool MHC>
__device__ __forceinline__ void demosaic_band_table(const BayerArgs &a, const uint8_t *table, const uint8_t *raw, uint8_t *dst, int band, uint8_t *lds)
{
    constexpr int R = MHC ? 2 : 1, NR = 2 * R + 1;
    const uint8_t *tab = lds;
    uint8_t *staged = lds + kBayerTableBytes;
    if (threadIdx.x < kBayerTableBytes / 16) reinterpret_cast<u32x4 *>(lds)[threadIdx.x] = reinterpret_cast<const u32x4 *>(table)[threadIdx.x];
    const int W = a.W, H = a.H;
    const int y0 = band * kBayerBandRows, y1 = min(y0 + kBayerBandRows, H);
    const int ylo = max(y0 - R, 0), yhi = min(y1 + R, H);   // staged rows [ylo, yhi): reflect-101 maps rows -R .. -1 and H .. H + R - 1 into them
    const int mis = stage_rows(raw + (size_t)ylo * W, (yhi - ylo) * W, staged);
    __syncthreads();

    const int nrun = (W + kRun - 1) / kRun;
    const int tasks = (y1 - y0) * nrun;
    const bool aligned = ((W | mis) & 15) == 0;
    for (int t = threadIdx.x; t < tasks; t += blockDim.x) {
        const int y = y0 + t / nrun, x0 = (t % nrun) * kRun;
        // p[k][j] = raw(row y - R + k, column x0 - R + j), j = 0 .. 15 + 2 R, reflect-101 at the frame's edges
        uint32_t p[NR][kRun + 2 * R];
#pragma unroll
        for (int k = 0; k < NR; k++) {
            int yy = y - R + k;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
            const uint8_t *r = staged + mis + (yy - ylo) * W;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int x = x0 - R + j;
                p[k][j] = r[x < 0 ? -x : x];
            }
            if (aligned && x0 + kRun <= W) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(r + x0);
#pragma unroll
                for (int j = 0; j < kRun; j++) p[k][j + R] = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
            } else {
#pragma unroll
                for (int j = 0; j < kRun; j++) {
                    const int x = x0 + j;
                    p[k][j + R] = r[x < W ? x : max(2 * W - 2 - x, 0)];   // (columns from W + R on belong to pixels that are not stored)
                }
            }
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int x = x0 + kRun + j;
                p[k][kRun + R + j] = r[x < W ? x : max(2 * W - 2 - x, 0)];
            }
        }
        const bool r_row = (y & 1) == a.ry;
        uint32_t out[3 * kRun];
#pragma unroll
        for (int j = 0; j < kRun; j++) {
            const bool r_col = (j & 1) == a.rx;   // (x0 is even: column parity = j & 1)
            uint32_t Rv, Gv, Bv;
            if constexpr (MHC) {
                const int q = j + 2;
                const int c = (int)p[2][q];
                const int ns1 = (int)(p[1][q] + p[3][q]), we1 = (int)(p[2][q - 1] + p[2][q + 1]);
                const int ns2 = (int)(p[0][q] + p[4][q]), we2 = (int)(p[2][q - 2] + p[2][q + 2]);
                const int x4 = (int)(p[1][q - 1] + p[1][q + 1] + p[3][q - 1] + p[3][q + 1]);
                auto fin = [](int s) { return (uint32_t)min(max((s + 8) >> 4, 0), 255); };
                if (r_row == r_col) {             // an R or a B site
                    const uint32_t g = fin(8 * c + 4 * (ns1 + we1) - 2 * (ns2 + we2));
                    const uint32_t o = fin(12 * c + 4 * x4 - 3 * (ns2 + we2));
                    Gv = g;
                    Rv = r_row ? (uint32_t)c : o;
                    Bv = r_row ? o : (uint32_t)c;
                } else {                          // a G site: one colour has its samples in this row, the other in this column
                    const uint32_t hr = fin(10 * c + 8 * we1 - 2 * x4 - 2 * we2 + ns2);
                    const uint32_t vr = fin(10 * c + 8 * ns1 - 2 * x4 - 2 * ns2 + we2);
                    Gv = (uint32_t)c;
                    Rv = r_row ? hr : vr;
                    Bv = r_row ? vr : hr;
                }
            } else {
                const uint32_t c = p[1][j + 1];
                const uint32_t cross = (p[0][j + 1] + p[2][j + 1] + p[1][j] + p[1][j + 2] + 2u) >> 2;
                const uint32_t diag = (p[0][j] + p[0][j + 2] + p[2][j] + p[2][j + 2] + 2u) >> 2;
                const uint32_t horiz = (p[1][j] + p[1][j + 2] + 1u) >> 1;
                const uint32_t vert = (p[0][j + 1] + p[2][j + 1] + 1u) >> 1;
                if (r_row == r_col) {
                    Gv = cross;
                    Rv = r_row ? c : diag;
                    Bv = r_row ? diag : c;
                } else {
                    Gv = c;
                    Rv = r_row ? horiz : vert;
                    Bv = r_row ? vert : horiz;
                }
            }
            out[3 * j + 0] = tab[Rv];
            out[3 * j + 1] = tab[256 + Gv];
            out[3 * j + 2] = tab[512 + Bv];
        }
        store_run(dst + ((size_t)y * W + x0) * 3, out, x0, W);
    }
}

__global__ __launch_bounds__(256) void bayer_demosaic_lut_kernel(BayerArgs a, const uint8_t *table)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.y;
    demosaic_band_table<false>(a, table, a.raw + (size_t)b * a.raw_slot_bytes, a.dst + (size_t)b * a.dst_slot_bytes, blockIdx.x, lds);
}

__global__ __launch_bounds__(256) void bayer_demosaic_mhc_kernel(BayerArgs a, const uint8_t *table)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.y;
    demosaic_band_table<true>(a, table, a.raw + (size_t)b * a.raw_slot_bytes, a.dst + (size_t)b * a.dst_slot_bytes, blockIdx.x, lds);
}

void launch_demosaic(const BayerArgs &a, int batch, hipStream_t s)
{
    const int bands = (a.H + kBayerBandRows - 1) / kBayerBandRows;
    const size_t lds = (size_t)(kBayerBandRows + 2) * a.W + 16;
    hipLaunchKernelGGL(bayer_demosaic_kernel, dim3(bands, batch), dim3(256), lds, s, a);
}

void launch_demosaic_table(const BayerArgs &a, const uint8_t *table, bool mhc, int batch, hipStream_t s)
{
    const int bands = (a.H + kBayerBandRows - 1) / kBayerBandRows;
    const size_t lds = (size_t)(kBayerBandRows + (mhc ? 4 : 2)) * a.W + 16 + kBayerTableBytes;
    if (mhc) hipLaunchKernelGGL(bayer_demosaic_mhc_kernel, dim3(bands, batch), dim3(256), lds, s, a, table);
    else hipLaunchKernelGGL(bayer_demosaic_lut_kernel, dim3(bands, batch), dim3(256), lds, s, a, table);
}

}  // namespace irmv
