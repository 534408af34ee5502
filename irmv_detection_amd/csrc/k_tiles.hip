// Tiled search for gfx950: the last node of a tiled step merges the result lists of its N window slots -- N overlapping
// crops of ONE frame -- into one list in full-frame coordinates (irmv_engine_submit_tiles / irmv_engine_merge_tiles;
// irmv_detection_amd/tiles.py is the bit-exact host reference).
//
// Plain fp32 arithmetic, compiled with -ffp-contract=off like k_post.hip: every value below is one rounded fp32 operation of
// the values irmv_engine_results returns, so kernel, host reference and numpy agree bit for bit.
//
//   coordinates  X = float(local) + float(corner): the one fp32 add irmv_engine_results does.  The corner is DATA, read from
//                the engine's corner table when the kernel runs (buffer coordinates there; result coordinates under rotate180
//                are full - corner - window), so a captured step follows a moved tile.
//   seam cut     a record is cut if its box comes within edge_margin of an edge of its tile that is not an edge of the frame.
//   order        (cut ascending, score descending, tile ascending, index ascending) as ONE 64-bit key, sorted in LDS.
//   walk         in that order a record is kept unless an already kept record of ANOTHER tile and the SAME class has
//                inter > ios_thr * min(area_a, area_b) with it (no division, the iou_gt pattern of k_post.hip); it stops at
//                max_det kept records.  Records of one tile never suppress each other: their own NMS has ruled on them.
//
// One workgroup of 1024 threads.  LDS: one 64-bit key per record padded to a power of two (at most 4096: 32 KB) and one box
// per (tile, index) (at most 16 x 256 x 16 B = 64 KB).  Every LDS word that is read has been written by this launch: keys
// [0, P) are all stored (records, then all-ones padding) before the sort touches them, and a box is read only through a key
// of a record, whose box was stored with it.  The walk runs on wave 0 alone with the kept list in REGISTERS (kept record j
// lives in lane j % 64, register j / 64; max_det <= 256 = 4 registers), so it needs neither LDS hand-over nor barriers.
#include "irmv_common.hpp"

namespace irmv {

constexpr int kTileThreads = 1024;

static size_t tile_lds_bytes(int count, int max_det)
{
    int P = 2;
    while (P < count * max_det) P <<= 1;
    return (size_t)P * 8 + (size_t)count * max_det * 16;
}

// order-preserving map of an fp32 to an unsigned: a < b  <=>  ord(a) < ord(b) (for -0 < +0 and NaNs by their bits: total)
__device__ __forceinline__ unsigned int float_ord(float v)
{
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool ios_gt(const f32x4 a, const f32x4 b, float thr)
{
    const float iw = fmaxf(0.f, fminf(a[2], b[2]) - fmaxf(a[0], b[0]));
    const float ih = fmaxf(0.f, fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
    const float inter = iw * ih;
    const float aa = (a[2] - a[0]) * (a[3] - a[1]);
    const float ab = (b[2] - b[0]) * (b[3] - b[1]);
    return inter > thr * fminf(aa, ab);
}

// key: bit 48 cut | bits 16..47 ~ord(score) | bits 12..15 tile | bits 4..11 index | bits 0..3 class (below the order: (tile,
// index) is unique)
__global__ __launch_bounds__(kTileThreads) void tile_merge_kernel(TileArgs a, int cap_p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];   // [cap_p]
    f32x4 *s_box = reinterpret_cast<f32x4 *>(s_keys + cap_p);                     // [count][max_det]
    __shared__ int s_n[kMaxTiles], s_off[kMaxTiles + 1];
    const int tid = threadIdx.x;
    const float ios_thr = a.params->ios_thr, margin = a.params->edge_margin;
    if (tid < a.count) {
        const int n = a.fout[a.first + tid].num_dets;
        s_n[tid] = min(max(n, 0), a.max_det);
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int t = 0; t < a.count; t++) { s_off[t] = o; o += s_n[t]; }
        s_off[a.count] = o;
    }
    __syncthreads();
    const int n_in = s_off[a.count];
    int P = 2;
    while (P < n_in) P <<= 1;   // (<= cap_p: n_in <= count * max_det)
    for (int i = tid; i < a.count * a.max_det; i += kTileThreads) {
        const int t = i / a.max_det, k = i - t * a.max_det;
        if (k >= s_n[t]) continue;
        const int slot = a.first + t;
        int2 org = a.win[slot];
        org.x = min(max(org.x, 0), a.full_w - a.win_w);   // (as window_crop_kernel reads it)
        org.y = min(max(org.y, 0), a.full_h - a.win_h);
        const int x0 = a.rotate180 ? a.full_w - org.x - a.win_w : org.x;
        const int y0 = a.rotate180 ? a.full_h - org.y - a.win_h : org.y;
        const DevDet &d = a.dets[(size_t)slot * a.max_det + k];
        const float fx = (float)x0, fy = (float)y0;
        const f32x4 b = {d.xyxy[0] + fx, d.xyxy[1] + fy, d.xyxy[2] + fx, d.xyxy[3] + fy};
        const bool cut = (x0 > 0 && b[0] < fx + margin) || (y0 > 0 && b[1] < fy + margin) ||
                         (x0 + a.win_w < a.full_w && b[2] > (float)(x0 + a.win_w) - margin) ||
                         (y0 + a.win_h < a.full_h && b[3] > (float)(y0 + a.win_h) - margin);
        const int cls = (d.cls >= 0 && d.cls < 14) ? d.cls : 14;   // irmv_det.class_id (IRMV_NUM_CLASSES = UNKNOWN)
        s_box[i] = b;
        s_keys[s_off[t] + k] = ((unsigned long long)(cut ? 1u : 0u) << 48) | ((unsigned long long)(~float_ord(d.score)) << 16) |
                               ((unsigned long long)t << 12) | ((unsigned long long)k << 4) | (unsigned long long)cls;
    }
    for (int i = n_in + tid; i < P; i += kTileThreads) s_keys[i] = ~0ull;
    __syncthreads();
    // bitonic sort of keys [0, P), ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kTileThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const unsigned long long x = s_keys[i], y = s_keys[l];
                const bool up = (i & k) == 0;
                if ((x > y) == up) { s_keys[i] = y; s_keys[l] = x; }
            }
            __syncthreads();
        }
    }
    if (tid >= 64) return;
    const int lane = tid;
    f32x4 kb[4];
    int km[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { kb[r] = (f32x4){0.f, 0.f, 0.f, 0.f}; km[r] = -1; }
    int nkept = 0;
    for (int i = 0; i < n_in && nkept < a.max_det; i++) {
        const unsigned long long key = s_keys[i];
        const int cls = (int)(key & 15u), k = (int)(key >> 4) & 255, t = (int)(key >> 12) & 15, cut = (int)(key >> 48) & 1;
        const f32x4 b = s_box[t * a.max_det + k];
        const int meta = t << 8 | cls;
        bool hit = false;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool have = r * 64 + lane < nkept;
            hit = hit || (have && (km[r] >> 8) != t && (km[r] & 255) == cls && ios_gt(b, kb[r], ios_thr));
        }
        if (__ballot(hit) != 0ull) continue;   // (wave-uniform)
        const int reg = nkept >> 6, owner = nkept & 63;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r == reg && lane == owner) { kb[r] = b; km[r] = meta; }
        if (lane == 0) {
            int *o = a.out->rec[nkept];
            o[0] = t; o[1] = k; o[2] = cut; o[3] = 0;
        }
        nkept++;
    }
    if (lane == 0) { a.out->n_kept = nkept; a.out->n_in = n_in; }
}

bool tile_merge_prepare()
{
    return raise_lds_limit<tile_merge_kernel>(tile_lds_bytes(kMaxTiles, kMaxDetCap));
}

void launch_tile_merge(const TileArgs &a, hipStream_t s)
{
    if (a.count < 1 || a.count > kMaxTiles || a.max_det < 1 || a.max_det > kMaxDetCap) return;
    int P = 2;
    while (P < a.count * a.max_det) P <<= 1;
    hipLaunchKernelGGL(tile_merge_kernel, dim3(1), dim3(kTileThreads), tile_lds_bytes(a.count, a.max_det), s, a, P);
}

}  // namespace irmv
