// Debug images (irmv_engine_render): the node's visualized and binary frames from the slot's device frame, in one launch.
// include/irmv_hip.h ("debug images") states the picture; irmv_detection_amd/render.py is the host reference, bit for bit.
//
// render_view<S>: a workgroup owns a 64 x 16 tile of OUTPUT pixels, a thread four neighbours of one row.
//   1. thread i looks at mark record i (at most kMaxDetCap = blockDim of them, integers in output pixels already) and appends
//      what can touch the tile -- extent plus thickness -- to two LDS lists: boxes with labels, and armors.  The lists are
//      unordered (an LDS counter each); a box entry carries its record's index, and a pixel takes the hit with the LARGEST
//      index, which is "later marks overwrite earlier ones".  Armor marks are all one colour and all lie under every box.
//   2. every pixel's base: the S x S block of the frame (rotation folded into the fetch, as the light kernel does) averaged,
//      or thresholded with the light kernel's gray expression and OR-ed.
//   3. only in a tile with a non-empty list: boxes and labels, else armors, over the base.
// LDS: both lists, the font and the counters, 16.7 KiB.  Every word read was written by this workgroup: the counters before
// the first barrier, the font whole, list entries only below their counter.
#include "irmv_common.hpp"

namespace irmv {

namespace {

// box and label of one list entry at output pixel (px, py): YoloEngine.visualize_bboxes / _draw_label, clamps included
template <int G> __device__ __forceinline__ bool box_hit(const int *m, const RenderFont &font, int px, int py, int ow, int oh)
{
    const int x1 = m[0], y1 = m[1], x2 = m[2], y2 = m[3];
    if (m[4] & kRenderBox) {
        const int x1c = max(min(x1, ow - 1), 0), x2c = max(min(x2, ow - 1), 0), y1c = max(min(y1, oh - 1), 0), y2c = max(min(y2, oh - 1), 0);
        if ((py == y1 || py == y1 + 1 || py == y2 || py == y2 - 1) && px >= x1c && px <= x2c) return true;
        if ((px == x1 || px == x1 + 1 || px == x2 || px == x2 - 1) && py >= y1c && py <= y2c) return true;
    }
    if (m[4] & kRenderLabel) {
        const int cls = m[5], u = px - x1, v = py - (y1 - 7 * G);
        if (u >= 0 && v >= 0 && v < 7 * G && u < (int)font.len[cls] * 6 * G) {
            const int k = u / (6 * G), c = (u % (6 * G)) / G;
            if (c < 5 && ((font.glyph[font.name[cls][k]][v / G] >> (4 - c)) & 1)) return true;
        }
    }
    return false;
}

// every pixel within distance 1 of the segment a-b; exact in 64-bit integers (coordinates are below 2^26 in magnitude)
__device__ __forceinline__ bool seg_hit(int ax, int ay, int bx, int by, int px, int py)
{
    if (px < min(ax, bx) - 1 || px > max(ax, bx) + 1 || py < min(ay, by) - 1 || py > max(ay, by) + 1) return false;
    const long long dx = (long long)bx - ax, dy = (long long)by - ay, qx = (long long)px - ax, qy = (long long)py - ay;
    const long long L2 = dx * dx + dy * dy, t = qx * dx + qy * dy;
    if (L2 == 0 || t < 0) return qx * qx + qy * qy <= 1;
    if (t > L2) {
        const long long rx = (long long)px - bx, ry = (long long)py - by;
        return rx * rx + ry * ry <= 1;
    }
    const long long c = qx * dy - qy * dx, ac = c < 0 ? -c : c;
    return ac < (1ll << 31) && ac * ac <= L2;   // (L2 < 2^54: a larger |c| cannot pass, and its square would not fit)
}

template <int R> __device__ __forceinline__ bool armor_hit(const int *m, int px, int py)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int dx = px - m[i], dy = py - m[4 + i];
        if (dx >= -R - 1 && dx <= R + 1 && dy >= -R - 1 && dy <= R + 1) {
            const int d = dx * dx + dy * dy - R * R;
            if (d >= -2 * R && d <= 2 * R) return true;
        }
    }
    // LB 0, LT 1, RT 2, RB 3: LT-LB, RT-RB, LT-RT, LB-RB
    return seg_hit(m[1], m[5], m[0], m[4], px, py) || seg_hit(m[2], m[6], m[3], m[7], px, py) ||
           seg_hit(m[1], m[5], m[2], m[6], px, py) || seg_hit(m[0], m[4], m[3], m[7], px, py);
}

template <int S> __device__ __forceinline__ void base_pixel(const RenderArgs &a, int x, int y, uint8_t *o)
{
    int sum[3] = {0, 0, 0};
    bool any = false;
#pragma unroll
    for (int dy = 0; dy < S; dy++)
#pragma unroll
        for (int dx = 0; dx < S; dx++) {
            int sx = x * S + dx, sy = y * S + dy;   // (< ow * S <= W, < oh * S <= H)
            if (a.rotate180) { sx = a.W - 1 - sx; sy = a.H - 1 - sy; }
            const uint8_t *p = a.frame + ((size_t)sy * a.W + sx) * 3;
            const int p0 = p[0], p1 = p[1], p2 = p[2];
            sum[0] += p0; sum[1] += p1; sum[2] += p2;
            any = any || ((p0 * 3735 + p1 * 19235 + p2 * 9798 + (1 << 14)) >> 15) > a.threshold;
        }
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = a.binary ? (any ? 255 : 0) : (uint8_t)((sum[c] + S * S / 2) / (S * S));
}

}  // namespace

template <int S> __global__ __launch_bounds__(256) void render_view(const RenderArgs a)
{
    constexpr int G = S == 1 ? 3 : (S == 2 ? 2 : 1);   // glyph cell
    constexpr int R = S == 1 ? 5 : (S == 2 ? 3 : 2);   // ring radius
    __shared__ int s_box[kMaxDetCap][8];    // x1, y1, x2, y2, flags, cls, record index, -
    __shared__ int s_arm[kMaxDetCap][8];    // px[4], py[4]
    __shared__ RenderFont s_font;
    __shared__ int s_nbox, s_narm;
    static_assert(sizeof(RenderFont) % 4 == 0, "copied by words");
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * kRenderTileW, ty0 = blockIdx.y * kRenderTileH;
    const int tx1 = min(tx0 + kRenderTileW, a.ow) - 1, ty1 = min(ty0 + kRenderTileH, a.oh) - 1;
    if (tid == 0) { s_nbox = 0; s_narm = 0; }
    for (int i = tid; i < (int)(sizeof(RenderFont) / 4); i += 256)
        reinterpret_cast<uint32_t *>(&s_font)[i] = reinterpret_cast<const uint32_t *>(a.font)[i];
    __syncthreads();
    if (tid < a.n) {
        const RenderMark m = a.marks[tid];
        int keep = 0;
        if (m.flags & kRenderBox) {
            const int x1c = max(min(m.x1, a.ow - 1), 0), x2c = max(min(m.x2, a.ow - 1), 0), y1c = max(min(m.y1, a.oh - 1), 0), y2c = max(min(m.y2, a.oh - 1), 0);
            const int lo_x = min(min(m.x1, m.x2 - 1), x1c), hi_x = max(max(m.x2, m.x1 + 1), x2c);
            const int lo_y = min(min(m.y1, m.y2 - 1), y1c), hi_y = max(max(m.y2, m.y1 + 1), y2c);
            if (lo_x <= tx1 && hi_x >= tx0 && lo_y <= ty1 && hi_y >= ty0) keep |= kRenderBox;
        }
        if (m.flags & kRenderLabel) {
            const int w = (int)s_font.len[m.cls] * 6 * G;
            if (m.x1 <= tx1 && m.x1 + w - 1 >= tx0 && m.y1 - 7 * G <= ty1 && m.y1 - 1 >= ty0) keep |= kRenderLabel;
        }
        if (keep) {
            int *d = s_box[atomicAdd(&s_nbox, 1)];
            d[0] = m.x1; d[1] = m.y1; d[2] = m.x2; d[3] = m.y2; d[4] = keep; d[5] = m.cls; d[6] = tid;
        }
        if (m.flags & kRenderArmor) {
            const int lo_x = min(min(m.px[0], m.px[1]), min(m.px[2], m.px[3])) - R - 1, hi_x = max(max(m.px[0], m.px[1]), max(m.px[2], m.px[3])) + R + 1;
            const int lo_y = min(min(m.py[0], m.py[1]), min(m.py[2], m.py[3])) - R - 1, hi_y = max(max(m.py[0], m.py[1]), max(m.py[2], m.py[3])) + R + 1;
            if (lo_x <= tx1 && hi_x >= tx0 && lo_y <= ty1 && hi_y >= ty0) {
                int *d = s_arm[atomicAdd(&s_narm, 1)];
#pragma unroll
                for (int i = 0; i < 4; i++) { d[i] = m.px[i]; d[4 + i] = m.py[i]; }
            }
        }
    }
    __syncthreads();
    const int x = tx0 + (tid & 15) * 4, y = ty0 + (tid >> 4);
    if (x >= a.ow || y >= a.oh) return;
    const int npx = min(4, a.ow - x), nbox = s_nbox, narm = s_narm;
    uint8_t o[12];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= npx) { o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0; continue; }
        base_pixel<S>(a, x + j, y, o + 3 * j);
        if (nbox | narm) {
            int best = -1, cls = 0;
            for (int k = 0; k < nbox; k++)
                if (s_box[k][6] > best && box_hit<G>(s_box[k], s_font, x + j, y, a.ow, a.oh)) { best = s_box[k][6]; cls = s_box[k][5]; }
            if (best >= 0) {
                o[3 * j] = cls < 7 ? 0 : 255; o[3 * j + 1] = 0; o[3 * j + 2] = cls < 7 ? 255 : 0;
            } else {
                for (int k = 0; k < narm; k++)
                    if (armor_hit<R>(s_arm[k], x + j, y)) { o[3 * j] = 0; o[3 * j + 1] = 255; o[3 * j + 2] = 0; break; }
            }
        }
    }
    uint8_t *q = a.dst + ((size_t)y * a.ow + x) * 3;
    if (npx == 4 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
#pragma unroll
        for (int w = 0; w < 3; w++)
            reinterpret_cast<uint32_t *>(q)[w] = (uint32_t)o[4 * w] | ((uint32_t)o[4 * w + 1] << 8) | ((uint32_t)o[4 * w + 2] << 16) | ((uint32_t)o[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++)
            if (i < 3 * npx) q[i] = o[i];
    }
}

void launch_render_view(const RenderArgs &a, hipStream_t s)
{
    const dim3 grid((a.ow + kRenderTileW - 1) / kRenderTileW, (a.oh + kRenderTileH - 1) / kRenderTileH);
    if (a.scale == 1) hipLaunchKernelGGL(render_view<1>, grid, dim3(256), 0, s, a);
    else if (a.scale == 2) hipLaunchKernelGGL(render_view<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(render_view<4>, grid, dim3(256), 0, s, a);
}

}  // namespace irmv
