// Frame metering for gfx950 (include/irmv_hip.h, "frame metering"): four 256-bin integer histograms of a rectangle of the
// slot's frame -- the view's HWC frame (channels as stored, and the light extraction's gray) or a Bayer engine's raw CFA frame
// (R, G, B sites and all sites).  Everything is an integer count, so the result does not depend on the order of the adds and
// irmv_detection_amd/metering.py reproduces it bit for bit.
//
// The rectangle, the step and the domain are DATA: both kernels read the MeterParams record and the slot's window corner from
// device memory when they run and compute the geometry themselves (meter_geometry, the function irmv_meter_map exports), so a
// captured graph holds addresses only and a new rectangle re-captures nothing.  params->on == 0: frame_meter_kernel returns at
// once and frame_meter_sum_kernel writes an all-zero record.
//
// frame_meter_kernel, grid (workgroups, frames), kMeterThreads threads.  A task is one sampled row of the region cut into
// segments of 64 lane-groups, one task per wave and trip (k_window.hip's layout).  A lane-group is what one lane loads with
// aligned 16-byte loads: VIEW 48 bytes = 16 whole pixels (the first group starts at the first pixel of the row whose address
// is a multiple of 16: at most 15 pixels in front of it), RAW 16 bytes = 8 CFA sites of one row.  The pixels in front of the
// first group and behind the last are read byte by byte by lanes of the row's segment 0.  No byte outside the region's rows
// [bx, bx + bw) is loaded: a group lies inside the row's span by construction.  Unsampled columns of a sampled row are
// loaded and skipped; unsampled rows are never touched.
// Each wave adds into a private [4][256] LDS histogram (ds_add_u32); they are summed per workgroup and the workgroup's
// partial goes to its place in the slab with plain vector stores.  Every workgroup of the grid writes its whole partial in
// every launch that is on, so the slab needs no reset.  frame_meter_sum_kernel, grid (frames), 1024 threads -- one bin each
// -- sums the launch's partials and writes the record: hist, n (the rows' sums), rect, domain, step.  No global atomics, no
// counter that outlives the launch.
// kFast: a lane-group whose pixels (RAW: cells) are all equal is added with four adds of its sample count instead of one add
// per sample -- the worst case is a uniform frame, every lane of every wave on one bin.  DESIGN.md section 23 has the
// measurements that chose it over merging runs of equal values one by one.
// Memory-bound: the sampled rows' bytes in; 4 KB per partial workgroup out and in again.
#include "irmv_common.hpp"

namespace irmv {

// The frame's geometry as both kernels see it; false: nothing to meter (off, an empty rectangle, RAW without a raw frame).
__device__ __forceinline__ bool meter_setup(const MeterArgs &a, int slot, MeterParams &p, MeterGeom &g)
{
    p = *a.params;
    g = MeterGeom{};
    if (!p.on) return false;
    p.domain = p.domain == kMeterRaw ? kMeterRaw : kMeterView;
    p.step = meter_step(p.step);
    if (p.domain == kMeterRaw && !a.raw) return false;
    int cx = 0, cy = 0;
    if (a.win) {   // (the host checks every corner it writes; a table entry cannot take the kernel out of its frame)
        const int2 o = a.win[slot];
        cx = min(max(o.x, 0), a.raw_w - a.vw);
        cy = min(max(o.y, 0), a.raw_h - a.vh);
    }
    g = meter_geometry(p, a.vw, a.vh, a.rotate180, cx, cy);
    return g.nx > 0 && g.ny > 0;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t *w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }
__device__ __forceinline__ uint32_t gray_of(uint32_t p0, uint32_t p1, uint32_t p2) { return (p0 * 3735u + p1 * 19235u + p2 * 9798u + (1u << 14)) >> 15; }   // the light extraction's
__device__ __forceinline__ void add_pixel(uint32_t *h, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t cnt)
{
    atomicAdd(&h[p0], cnt); atomicAdd(&h[256u + p1], cnt); atomicAdd(&h[512u + p2], cnt);
    atomicAdd(&h[768u + gray_of(p0, p1, p2)], cnt);
}
// how many of the n consecutive indices i0, i0 + 1, ... have ((i - ph) & m) == 0 (m + 1 a power of two)
__device__ __forceinline__ uint32_t sampled_in(int i0, int n, int ph, int m)
{
    const int first = (ph - i0) & m;
    return first < n ? (uint32_t)((n - first + m) / (m + 1)) : 0u;
}

template <bool kFast> __device__ __forceinline__ void meter_view_rows(const MeterArgs &a, int slot, const MeterGeom &g, int st, uint32_t *h)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint8_t *frame = a.frames + (size_t)slot * a.frame_bytes;
    const size_t pitch = (size_t)a.vw * 3;
    const int nseg = max(1, (g.bw / 16 + 63) / 64);   // segments per row: enough for its groups whatever the row's alignment
    const int tasks = g.ny * nseg;
    const int m = st - 1;                             // column q (from the region's first) is sampled iff ((q - px) & m) == 0
    for (int t = blockIdx.x * kMeterWaves + wave; t < tasks; t += gridDim.x * kMeterWaves) {
        const int r = t / nseg, seg = t - r * nseg;
        const uint8_t *s = frame + (size_t)(g.by + g.py + r * st) * pitch + (size_t)g.bx * 3;
        // pixels in front of the first 16-byte aligned pixel start: 3 k = -address (mod 16), and 3 * 11 = 1 (mod 16)
        const int head = min((int)((((16u - ((uint32_t)(uintptr_t)s & 15u)) & 15u) * 11u) & 15u), g.bw);
        const int nbody = (g.bw - head) >> 4;
        const int tail0 = head + (nbody << 4);
        if (seg == 0) {   // the row's ends: lanes 0..14 in front, lanes 16..30 behind
            const int q = lane < 16 ? lane : tail0 + lane - 16;
            const bool in = lane < 16 ? lane < head : (lane < 32 && q < g.bw);
            if (in && ((q - g.px) & m) == 0) add_pixel(h, s[3 * q], s[3 * q + 1], s[3 * q + 2], 1u);
        }
        const int c = seg * 64 + lane;
        if (c >= nbody) continue;
        const int q0 = head + 16 * c;
        const u32x4 *gp = reinterpret_cast<const u32x4 *>(s + 3 * (size_t)q0);
        const u32x4 v0 = gp[0], v1 = gp[1], v2 = gp[2];
        const uint32_t w[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
        if (kFast) {   // sixteen times one pixel: its three dwords repeat, and they are that pixel's bytes in rotation
            const uint32_t p0 = w[0] & 255u, p1 = (w[0] >> 8) & 255u, p2 = (w[0] >> 16) & 255u;
            bool same = w[0] == (p0 | p1 << 8 | p2 << 16 | p0 << 24) && w[1] == (p1 | p2 << 8 | p0 << 16 | p1 << 24) && w[2] == (p2 | p0 << 8 | p1 << 16 | p2 << 24);
#pragma unroll
            for (int i = 3; i < 12; i++) same = same && w[i] == w[i - 3];
            if (same) {
                const uint32_t cnt = sampled_in(q0, 16, g.px, m);
                if (cnt) add_pixel(h, p0, p1, p2, cnt);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (((q0 + k - g.px) & m) == 0) add_pixel(h, byte_of(w, 3 * k), byte_of(w, 3 * k + 1), byte_of(w, 3 * k + 2), 1u);
    }
}

template <bool kFast> __device__ __forceinline__ void meter_raw_rows(const MeterArgs &a, int slot, const MeterGeom &g, int st, uint32_t *h)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint8_t *frame = a.raw + (size_t)slot * a.raw_bytes;
    const size_t pitch = (size_t)a.raw_w;
    const int n = g.bw;                               // sites (bytes) of a row of the region
    const int nseg = max(1, (n / 16 + 63) / 64);
    const int tasks = 2 * g.ny * nseg;                // both rows of every sampled cell row
    const int m = st - 1;                             // site q is sampled iff its cell q >> 1 is: ((q >> 1) & m) == 0
    for (int t = blockIdx.x * kMeterWaves + wave; t < tasks; t += gridDim.x * kMeterWaves) {
        const int r = t / nseg, seg = t - r * nseg;
        const int y = g.by + 2 * (r >> 1) * st + (r & 1);
        const uint8_t *s = frame + (size_t)y * pitch + (size_t)g.bx;
        // the colour row (0 R, 1 G, 2 B) of the sites at even and at odd x of this row, times 256
        const bool ry = (y & 1) == a.ry;
        const uint32_t row_at[2] = {256u * (uint32_t)(ry ? ((0 == a.rx) ? 0 : 1) : ((0 == a.rx) ? 1 : 2)),
                                    256u * (uint32_t)(ry ? ((1 == a.rx) ? 0 : 1) : ((1 == a.rx) ? 1 : 2))};
        const int head = min((int)((16u - ((uint32_t)(uintptr_t)s & 15u)) & 15u), n);
        const int nbody = (n - head) >> 4;
        const int tail0 = head + (nbody << 4);
        if (seg == 0) {
            const int q = lane < 16 ? lane : tail0 + lane - 16;
            const bool in = lane < 16 ? lane < head : (lane < 32 && q < n);
            if (in && ((q >> 1) & m) == 0) {
                const uint32_t v = s[q];
                atomicAdd(&h[((g.bx + q) & 1 ? row_at[1] : row_at[0]) + v], 1u);
                atomicAdd(&h[768u + v], 1u);
            }
        }
        const int c = seg * 64 + lane;
        if (c >= nbody) continue;
        const int q0 = head + 16 * c;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(s + q0);
        const uint32_t w[4] = {v[0], v[1], v[2], v[3]};
        const int odd = (g.bx + q0) & 1;              // x parity of the group's first site; alternates from there
        const uint32_t row_e = odd ? row_at[1] : row_at[0], row_o = odd ? row_at[0] : row_at[1];
        if (kFast && !(q0 & 1)) {   // eight times one cell row: (b0, b1) repeated
            const uint32_t b0 = w[0] & 255u, b1 = (w[0] >> 8) & 255u;
            if (w[0] == (b0 | b1 << 8 | b0 << 16 | b1 << 24) && w[1] == w[0] && w[2] == w[0] && w[3] == w[0]) {
                const uint32_t cnt = sampled_in(q0 >> 1, 8, 0, m);
                if (cnt) {
                    atomicAdd(&h[row_e + b0], cnt); atomicAdd(&h[row_o + b1], cnt);
                    atomicAdd(&h[768u + b0], cnt); atomicAdd(&h[768u + b1], cnt);
                }
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < 16; k++)
            if ((((q0 + k) >> 1) & m) == 0) {
                const uint32_t b = byte_of(w, k);
                atomicAdd(&h[((k & 1) ? row_o : row_e) + b], 1u);
                atomicAdd(&h[768u + b], 1u);
            }
    }
}

// grid (workgroups, frames)
template <bool kFast> __global__ __launch_bounds__(kMeterThreads) void frame_meter_kernel(MeterArgs a)
{
    __shared__ uint32_t sh[kMeterWaves][1024];
    static_assert(sizeof sh == kMeterLdsBytes, "irmv_meter_limits reports the kernel's LDS");
    const int slot = a.first + blockIdx.y;
    MeterParams p;
    MeterGeom g;
    const bool active = meter_setup(a, slot, p, g);
    if (!p.on) return;   // (the same in every thread: off -- the sum kernel reads no partial)
#pragma unroll
    for (int i = 0; i < kMeterWaves * 1024 / kMeterThreads; i++) (&sh[0][0])[i * kMeterThreads + threadIdx.x] = 0u;
    __syncthreads();
    if (active) {
        if (p.domain == kMeterRaw) meter_raw_rows<kFast>(a, slot, g, p.step, sh[threadIdx.x >> 6]);
        else meter_view_rows<kFast>(a, slot, g, p.step, sh[threadIdx.x >> 6]);
    }
    __syncthreads();
    uint32_t *part = a.slab + ((size_t)slot * kMeterBlocksMax + min((int)blockIdx.x, kMeterBlocksMax - 1)) * 1024;
#pragma unroll
    for (int i = 0; i < 1024 / kMeterThreads; i++) {
        const int bin = i * kMeterThreads + threadIdx.x;
        uint32_t v = 0u;
#pragma unroll
        for (int wv = 0; wv < kMeterWaves; wv++) v += sh[wv][bin];
        part[bin] = v;
    }
}

// grid (frames), 1024 threads: thread t owns bin t of the [4][256] record; blocks = the partial workgroups of the launch
__global__ __launch_bounds__(1024) void frame_meter_sum_kernel(MeterArgs a, int blocks)
{
    __shared__ uint32_t wsum[16];
    const int slot = a.first + blockIdx.x, t = threadIdx.x;
    MeterStats &out = a.out[blockIdx.x];
    MeterParams p;
    MeterGeom g;
    const bool active = meter_setup(a, slot, p, g);
    uint32_t v = 0u;
    if (active) {
        const uint32_t *part = a.slab + (size_t)slot * kMeterBlocksMax * 1024 + t;
        const int nb = min(max(blocks, 0), kMeterBlocksMax);
#pragma unroll 16
        for (int b = 0; b < nb; b++) v += part[(size_t)b * 1024];
    }
    (&out.hist[0][0])[t] = v;
    uint32_t s = v;   // n[row]: the row's 256 bins are four whole waves
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t < 4) out.n[t] = wsum[4 * t] + wsum[4 * t + 1] + wsum[4 * t + 2] + wsum[4 * t + 3];
    else if (t == 64) {   // (static indices: a runtime one would put g in LDS)
        out.rect[0] = g.rect[0]; out.rect[1] = g.rect[1]; out.rect[2] = g.rect[2]; out.rect[3] = g.rect[3];
        out.domain = p.on ? p.domain : 0;
        out.step = p.on ? p.step : 0;
        out.pad_[0] = out.pad_[1] = 0;
    }
}

void launch_frame_meter(const MeterArgs &a, int batch, bool fast, hipStream_t s)
{
    if (batch <= 0) return;
    const int blocks = meter_blocks(a.vh, batch);
    if (fast) hipLaunchKernelGGL(frame_meter_kernel<true>, dim3(blocks, batch), dim3(kMeterThreads), 0, s, a);
    else hipLaunchKernelGGL(frame_meter_kernel<false>, dim3(blocks, batch), dim3(kMeterThreads), 0, s, a);
    hipLaunchKernelGGL(frame_meter_sum_kernel, dim3(batch), dim3(1024), 0, s, a, blocks);
}

}  // namespace irmv
