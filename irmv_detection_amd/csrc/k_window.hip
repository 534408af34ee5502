// Tracking window for gfx950: the first op of a window engine's step cuts the slot's win_w x win_h window out of its full HWC
// frame into the compact frame every later kernel reads (front_fused / preprocess, rotate180, the light extraction), so
// that to them a window engine is an engine whose source frame is the window.
//
// The window's corner is DATA: the kernel reads (bx0, by0) of its slot from a device table when it runs, so a captured
// graph holds the table's pointer and never the position -- moving the window re-captures nothing.
//
// Work layout: a task is 64 consecutive 16-byte chunks of one destination row, one task per wave and trip.  A window row
// is contiguous in the source and in the destination, but the two sit at different offsets modulo 16 (the source row starts
// at (by0 + r) * 3 full_w + 3 bx0, any residue; the destination row at r * 3 win_w).  The destination decides the chunking:
// up to 15 bytes in front of the row's first aligned destination chunk and behind its last are copied byte by byte, and
// every chunk between is ONE aligned 16-byte store.  Its 16 source bytes straddle two aligned source chunks at a byte shift
// m that is the same for the whole wave (the lanes' addresses differ by 16): lane i loads the aligned chunk that holds its
// first byte -- one 16-byte load per lane, each source byte fetched once, which matters when the source is the pinned host
// slot across PCIe --, takes the next chunk from lane i + 1 by a wave shuffle, and funnel-shifts the pair by m
// (v_alignbyte_b32).  The lane behind the row's last chunk loads the chunk that one needs; lane 63 has no lane to its right and
// loads its next chunk itself (one load in 64 twice).
//
// Bounds: an aligned source chunk may begin up to 15 bytes in front of the bytes a lane needs and end up to 15 behind them.
// A chunk that would leave the slot's full frame [frame, frame + 3 full_w full_h) is not loaded: the destination chunk it
// would have fed is copied byte by byte instead (this can only be the first and the last chunk of a frame).  A tiled step
// (CropArgs::src_slot >= 0) cuts every slot's window out of ONE slot's frame: `frame` and `frame_end` are then that slot's.
// Stores stay inside the slot's window frame by construction: rows r < win_h, bytes < 3 win_w of each.
// Memory-bound: 3 win_w win_h bytes in, the same out.
#include "irmv_common.hpp"

namespace irmv {

constexpr int kCropBlocksMax = 256;   // workgroups per frame: one frame alone still reaches every CU

__device__ __forceinline__ u32x4 shfl_down1(const u32x4 v)
{
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = (unsigned int)__shfl_down((int)v[i], 1);
    return r;
}

// bytes [m, m + 16) of the 32 bytes lo : hi, m in [1, 15] and the same for every lane of the wave
__device__ __forceinline__ u32x4 funnel(const u32x4 lo, const u32x4 hi, int m)
{
    const unsigned int x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const unsigned int sh = (unsigned int)m & 3u;
    u32x4 o;
    switch (m >> 2) {   // (static register indices in every arm: a runtime index would put x in scratch)
    case 0:
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = __builtin_amdgcn_alignbyte(x[w + 1], x[w], sh);
        break;
    case 1:
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = __builtin_amdgcn_alignbyte(x[w + 2], x[w + 1], sh);
        break;
    case 2:
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = __builtin_amdgcn_alignbyte(x[w + 3], x[w + 2], sh);
        break;
    default:
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = __builtin_amdgcn_alignbyte(x[w + 4], x[w + 3], sh);
        break;
    }
    return o;
}

// grid (workgroups, frames)
__global__ __launch_bounds__(256) void window_crop_kernel(CropArgs a)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int slot = a.first + b;
    int2 org = a.win[slot];
    org.x = min(max(org.x, 0), a.full_w - a.win_w);   // (the host checks every origin it writes; a table entry cannot take the kernel out of its frame)
    org.y = min(max(org.y, 0), a.full_h - a.win_h);
    // a tiled step cuts every slot's window out of ONE slot's frame; the bounds below follow that frame
    const uint8_t *frame = a.src + (size_t)(a.src_slot >= 0 ? a.src_slot : slot) * a.src_slot_bytes;
    const uint8_t *frame_end = frame + (size_t)a.full_w * a.full_h * 3;
    uint8_t *out = a.dst + (size_t)slot * a.dst_slot_bytes;
    const int n = a.win_w * 3;                       // bytes of a window row
    const size_t pitch = (size_t)a.full_w * 3;
    const int nseg = max(1, (n / 16 + 63) / 64);     // tasks per row: enough for its aligned chunks whatever the row's alignment
    const int tasks = a.win_h * nseg;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < tasks; t += gridDim.x * 4) {
        const int r = t / nseg, seg = t - r * nseg;
        const uint8_t *s = frame + (size_t)(org.y + r) * pitch + (size_t)org.x * 3;
        uint8_t *d = out + (size_t)r * n;
        const int head = min((int)((16 - ((uintptr_t)d & 15)) & 15), n);
        const int nbody = (n - head) >> 4;
        const int tail0 = head + (nbody << 4);
        if (seg == 0) {   // the row's unaligned ends: lanes 0..14 in front, lanes 16..30 behind
            if (lane < head) d[lane] = s[lane];
            const int k = tail0 + lane - 16;
            if (lane >= 16 && k < n) d[k] = s[k];
        }
        if (seg * 64 >= nbody) continue;             // (wave-uniform)
        const int c = seg * 64 + lane;
        const bool valid = c < nbody;
        const uint8_t *sp = s + head + 16 * (size_t)c;
        const int m = (int)((uintptr_t)sp & 15);     // the same in every lane
        const uint8_t *al = sp - m;
        // the aligned source chunk of this lane's first byte; chunk nbody is loaded too (its left neighbour's second half)
        const bool have = c <= nbody && al >= frame && al + 16 <= frame_end;
        u32x4 lo = (u32x4){0u, 0u, 0u, 0u};
        if (have) lo = *reinterpret_cast<const u32x4 *>(al);
        u32x4 hi = shfl_down1(lo);
        bool have_hi = __shfl_down((int)have, 1) != 0;
        if (lane == 63 && valid && m != 0) {         // no lane to its right
            have_hi = al + 32 <= frame_end;
            if (have_hi) hi = *reinterpret_cast<const u32x4 *>(al + 16);
        }
        if (!valid) continue;
        uint8_t *dp = d + head + 16 * (size_t)c;
        if (m == 0 && have) *reinterpret_cast<u32x4 *>(dp) = lo;
        else if (m != 0 && have && have_hi) *reinterpret_cast<u32x4 *>(dp) = funnel(lo, hi, m);
        else {
#pragma unroll
            for (int k = 0; k < 16; k++) dp[k] = sp[k];
        }
    }
}

void launch_window_crop(const CropArgs &a, int batch, hipStream_t s)
{
    if (batch <= 0) return;
    const int nseg = (a.win_w * 3 / 16 + 63) / 64 > 0 ? (a.win_w * 3 / 16 + 63) / 64 : 1;
    const int tasks4 = (a.win_h * nseg + 3) / 4;
    const int blocks = tasks4 < kCropBlocksMax ? tasks4 : kCropBlocksMax;
    hipLaunchKernelGGL(window_crop_kernel, dim3(blocks, batch), dim3(256), 0, s, a);
}

}  // namespace irmv
