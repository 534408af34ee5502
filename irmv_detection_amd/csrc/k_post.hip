// Detection post-processing on the GPU: DFL box decode + score filter, score
// sort, class-aware greedy NMS, keypoint decode, parse_output scaling and planar
// (IPPE) PnP -- everything the reference does after the conv body:
//   EfficientNMS_TRT plugin   (bound at src/yolo_engine.cpp:53-57,82-85)
//   YoloEngine::parse_output  (src/yolo_engine.cpp:202-220)
//   PnPSolver::solvePnP       (src/pnp_solver.cpp:36-52, cv::SOLVEPNP_IPPE)
//   Rodrigues -> quaternion   (src/irm_detector.cpp:218-226)
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the fp32 decode / IoU
// expressions are evaluated exactly as written (fmaf only where spelled out), so
// candidate sets, sort order and NMS survivors are bit-reproducible against the
// CPU oracle on identical head tensors.
//
// Latency-bound integer/compare work: one lane per anchor for the decode, one
// workgroup per frame for sort + NMS, the IoU test of a 64-candidate block
// against the kept set and against itself done wave-wide with ballots.
//
// This file is compiled TWICE.  On its own it holds every kernel and launcher an engine has always run.  k_post_alt.hip includes
// it with IRMV_ALT_TU defined and takes only the templates and device functions, to instantiate nms_pnp_kernel<true> and the
// two-solution PnP kernel in a module of their own: with both instantiations in one module the inliner's choices for
// nms_pnp_kernel<false> changed when the template parameter came (13 333 -> 13 494 instructions) -- alone in its module it was,
// instruction for instruction, the kernel from before.  (This build, every phase a __forceinline__ function: 12 896
// instructions for <false>, 13 106 for <true>, as scripts/isa_stats.py matches them; profiles/post_refactor_ab.txt.)
#include "irmv_common.hpp"
#include "pnp_device.hpp"

namespace irmv {

// exp(x) as a fixed sequence of fp32 operations (same sequence in oracle/orc_post.c)
__device__ __forceinline__ float irmv_expf(float x)
{
    x = x < -87.0f ? -87.0f : x;
    x = x > 88.0f ? 88.0f : x;
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);
    r = fmaf(n, -1.42860682030941723212e-6f, r);
    float p = 1.0f / 720.0f;
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return __int_as_float(__float_as_int(p) + ((int)n << 23));
}

__device__ __forceinline__ uint32_t orderable(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unorderable(uint32_t u)
{
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// Anchor of a candidate key's id (= anchor * nc + class), CLAMPED to the head: keys are only ever written with valid ids, but
// a key list read to a count that held garbage hands stale bytes to every later phase, and none of
// them may turn that into an access outside a buffer.
__device__ __forceinline__ int anchor_of(uint32_t id, int nc, int A)
{
    const uint32_t an = id / (uint32_t)nc;
    return an < (uint32_t)A ? (int)an : A - 1;
}

// A candidate key is (orderable class logit) << 32 | (0xffffffff - id), id = anchor * nc + class: larger key = better score, and
// among equal scores the smaller (anchor, class).  pack_key writes it, unpack_key reads its lower half back.
__device__ __forceinline__ unsigned long long pack_key(float logit, int an, int nc, int c)
{
    return ((unsigned long long)orderable(logit) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(an * nc + c));
}
struct KeyId { uint32_t id; int an, cls; };      // id, anchor (clamped: anchor_of), class
__device__ __forceinline__ KeyId unpack_key(unsigned long long key, int nc, int A)
{
    const uint32_t id = 0xffffffffu - (uint32_t)(key & 0xffffffffu);
    return KeyId{id, anchor_of(id, nc, A), (int)(id % (uint32_t)nc)};
}

// anchor -> grid position, stride, and the (level base, level size, index in level) that locate its head record
__device__ __forceinline__ void anchor_geom(int a, int net_w, int net_h, int &ix, int &iy, int &stride, int &lbase, int &lhw, int &rin)
{
    int base = 0;
    ix = iy = 0;
    stride = 0;
    lbase = 0;
    lhw = 1;
    rin = 0;
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const int s = 8 << l, w = net_w / s, cnt = w * (net_h / s);
        if (stride == 0 && a < base + cnt) {
            const int r = a - base;
            iy = r / w;
            ix = r - iy * w;
            stride = s;
            lbase = base;
            lhw = cnt;
            rin = r;
        }
        base += cnt;
    }
}

__device__ __forceinline__ const float *head_rec(const float *head_all, int slots_total, int slot, int lbase, int lhw, int rin)
{
    return head_all + ((size_t)lbase * slots_total + (size_t)slot * lhw + rin) * kHeadRec;
}

// the head record of an anchor of frame b
__device__ __forceinline__ const float *anchor_rec(const PostArgs &a, int b, int an)
{
    int ix, iy, s, lbase, lhw, rin;
    anchor_geom(an, a.net_w, a.net_h, ix, iy, s, lbase, lhw, rin);
    return head_rec(a.head_all, a.slots_total, a.first + b, lbase, lhw, rin);
}

__device__ __forceinline__ float dfl_side(const float *l)
{
    float m = l[0];
#pragma unroll
    for (int j = 1; j < 16; j++) m = l[j] > m ? l[j] : m;
    float se = 0.0f, sj = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const float e = irmv_expf(l[j] - m);
        se = se + e;
        sj = sj + e * (float)j;
    }
    return sj / se;
}

// side q's sixteen DFL logits of a head record, as the four 16-byte reads every decoder issues (when, and how many rounds
// of them together, is the caller's business)
__device__ __forceinline__ void load_dfl(const float *rec, int q, f32x4 v[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = reinterpret_cast<const f32x4 *>(rec + 16 * q)[i];
}

// The box of anchor `an` from its 4 x 16 DFL logits, a quad of lanes per anchor: lane q of the quad hands in side q's logits
// (load_dfl), and the box comes back ON LANE q == 0 (zeros elsewhere).  The four lanes of a quad must be active together.
__device__ __forceinline__ f32x4 box_from_dfl(const f32x4 v[4], int an, int lane, int net_w, int net_h)
{
    const int base = lane & ~3;
    float l[16];
#pragma unroll
    for (int i = 0; i < 4; i++) { l[4 * i] = v[i][0]; l[4 * i + 1] = v[i][1]; l[4 * i + 2] = v[i][2]; l[4 * i + 3] = v[i][3]; }
    const float d = dfl_side(l);
    const float dl = __shfl(d, base), dt = __shfl(d, base + 1), dr = __shfl(d, base + 2), db = __shfl(d, base + 3);
    f32x4 box = {0.f, 0.f, 0.f, 0.f};
    if ((lane & 3) == 0) {
        int ix, iy, s, lbase, lhw, rin;
        anchor_geom(an, net_w, net_h, ix, iy, s, lbase, lhw, rin);
        const float ax = (float)ix + 0.5f, ay = (float)iy + 0.5f, sf = (float)s;
        box[0] = (ax - dl) * sf;
        box[1] = (ay - dt) * sf;
        box[2] = (ax + dr) * sf;
        box[3] = (ay + db) * sf;
    }
    return box;
}

// Decode phase of nms_pnp_kernel, part 1 (scan): one quad of lanes per anchor, lane q owns classes 4q..4q+3 (one 16-byte
// read of the record's class logits).  Candidate keys go to the workgroup's LDS list (and to the frame's global list,
// which only the > kCandCap path reads back); anchors with at least one candidate are appended to `alist`.  List
// positions come from LDS counters: no global atomic, no counter that outlives the kernel.
__device__ __forceinline__ void scan_quad(const PostArgs &a, float min_thr, int an, bool live, const f32x4 cl, unsigned long long *skeys, unsigned long long *gk,
                                          int *s_ncand, unsigned short *alist, int *s_nanch)
{
    const int q = threadIdx.x & 3;
    bool hit = false;
#pragma unroll
    for (int i = 0; i < 4; i++) hit = hit || (live && 4 * q + i < a.nc && cl[i] > min_thr);
    if (!__any(hit)) return;                      // the common case: nothing in these 16 anchors
    // class policy: behind the pre-test against the smallest threshold, the lane's own four classes against their own
    const f32x4 th = *reinterpret_cast<const f32x4 *>(a.cls->thr + 4 * q);
    hit = false;
#pragma unroll
    for (int i = 0; i < 4; i++) hit = hit || (live && 4 * q + i < a.nc && cl[i] > th[i]);
    if (!__any(hit)) return;
    const int lane = threadIdx.x & 63, base = lane & ~3;
    const bool quad_hit = ((__ballot(hit) >> base) & 0xfull) != 0ull;
    if (alist && quad_hit && q == 0) alist[atomicAdd(s_nanch, 1)] = (unsigned short)an;
    if (!hit) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c = 4 * q + i;
        const float logit = cl[i];
        if (c < a.nc && logit > th[i]) {
            const int idx = atomicAdd(s_ncand, 1);   // LDS; <= A * nc = key_cap by construction
            const unsigned long long key = pack_key(logit, an, a.nc, c);
            if (idx < kCandCap) skeys[idx] = key;
            gk[idx] = key;
        }
    }
}

// part 2: the box of every anchor on `alist`, four lanes per anchor, lane q decoding side q (16 DFL logits, one 64-byte
// read).  Boxes exist only where the NMS walk can read them: 5/6 of the head's bytes are never touched.
__device__ __forceinline__ void decode_boxes(const PostArgs &a, int b, const unsigned short *alist, int n_anch)
{
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63;
    for (int i0 = 0; i0 < n_anch; i0 += 256) {
        const int ai = i0 + (threadIdx.x >> 2);
        const bool live = ai < n_anch;                 // quad-uniform
        const int an = live ? (alist ? (int)alist[ai] : ai) : 0;   // no list (more anchors than it can index): every anchor
        f32x4 v[4];
        load_dfl(anchor_rec(a, b, an), q, v);
        const f32x4 box = box_from_dfl(v, an, lane, a.net_w, a.net_h);
        if (live && q == 0) reinterpret_cast<f32x4 *>(a.boxes)[(size_t)b * a.A + an] = box;
    }
}

// ---------------------------------------------------------------------------
// Scan + box decode as a kernel of its own, kScanBlocks workgroups per frame.  One workgroup reading a frame's class
// logits (8400 x 64 B, strided through 384-byte records) is bound by what ONE CU can pull from memory (~30 GB/s): 18 of
// the 53 us of a single-frame nms_pnp launch, 25 - 30 of 98 us with 64 frames on 64 CUs.  Spread over 16 CUs per frame
// the same bytes take ~2 us.  Keys go to the frame's global list in whatever order the workgroups append them (the
// sort of nms_pnp_kernel makes the order irrelevant: keys are unique); the box of every anchor with a candidate is
// decoded here, four lanes per anchor, exactly as decode_boxes does.
// ---------------------------------------------------------------------------
constexpr int kScanU = 2;   // loads in flight per lane: one memory round trip per U * 64 anchors
#ifndef IRMV_ALT_TU
// A workgroup's range of (anchor, side) quads: a kScanBlocks-th of the frame, unless its keys would not fit in LDS (nets of more
// than 22 528 anchors, beyond 1024 x 1024, whose launch was refused): then ranges that do, and as many more workgroups.
static int scan_quads_per_block(int A, int nc)
{
    constexpr int step = 256 * kScanU;
    const int per = ((A * 4 + kScanBlocks - 1) / kScanBlocks + step - 1) / step * step;
    const int cap = (int)(kScanLdsMax / (nc * sizeof(unsigned long long))) * 4 / step * step;
    return per < cap ? per : cap;
}

// The workgroup's keys are collected in LDS (sized for every (anchor, class) pair of its range: it cannot overflow) and
// leave with ONE global atomic per workgroup: one atomic per candidate on the frame's counter serialises in L2 (measured:
// ~40 ns each, 15 us for 380 candidates -- as long as the scan this kernel was split off to shorten).
__global__ __launch_bounds__(256) void scan_decode_kernel(PostArgs a, int per)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];
    __shared__ int s_n, s_base;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, q = tid & 3, base = lane & ~3;
    const int quads = a.A * 4;
    constexpr int U = kScanU;
    if (tid == 0) s_n = 0;
    const float min_thr = a.cls->min_thr;   // class policy: the smallest per-class threshold (uniform: one scalar load)
    __syncthreads();
    const int w0 = a.net_w >> 3, h0 = a.net_h >> 3, A0 = w0 * h0, A1 = A0 + (w0 >> 1) * (h0 >> 1);   // level boundaries
    unsigned long long *gk = a.keys + (size_t)b * a.key_cap;
    const int t_end = min((int)(blockIdx.x + 1) * per, quads);
    for (int t0 = blockIdx.x * per; t0 < t_end; t0 += 256 * U) {
        f32x4 cl[U];
        const float *rec[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = t0 + u * 256 + tid;
            const int an = t < quads ? (t >> 2) : 0;
            const int lbase = an < A0 ? 0 : (an < A1 ? A0 : A1), lhw = an < A0 ? A0 : (an < A1 ? A1 - A0 : a.A - A1);
            rec[u] = head_rec(a.head_all, a.slots_total, a.first + b, lbase, lhw, an - lbase);
            cl[u] = reinterpret_cast<const f32x4 *>(rec[u] + kClsOff)[q];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = t0 + u * 256 + tid;
            const bool live = t < quads;
            const int an = live ? (t >> 2) : 0;
            bool hit = false;
#pragma unroll
            for (int i = 0; i < 4; i++) hit = hit || (live && 4 * q + i < a.nc && cl[u][i] > min_thr);
            if (__ballot(hit) == 0ull) continue;                   // the common case: nothing in these 16 anchors
            // ... behind that pre-test, rarely: the lane's own four classes against their own thresholds
            const f32x4 th = reinterpret_cast<const f32x4 *>(a.cls->thr)[q];
            hit = false;
#pragma unroll
            for (int i = 0; i < 4; i++) hit = hit || (live && 4 * q + i < a.nc && cl[u][i] > th[i]);
            const unsigned long long hits = __ballot(hit);
            if (hits == 0ull) continue;
            if (hit) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int c = 4 * q + i;
                    if (c < a.nc && cl[u][i] > th[i]) s_keys[atomicAdd(&s_n, 1)] = pack_key(cl[u][i], an, a.nc, c);
                }
            }
            if (((hits >> base) & 0xfull) != 0ull) {               // this quad's anchor has a candidate: its box, side q on lane q
                // (shuffles inside a divergent region: the four lanes of a quad are active together by construction)
                f32x4 v[4];
                load_dfl(rec[u], q, v);
                const f32x4 box = box_from_dfl(v, an, lane, a.net_w, a.net_h);
                if (q == 0) reinterpret_cast<f32x4 *>(a.boxes)[(size_t)b * a.A + an] = box;
            }
        }
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;
    if (tid == 0) s_base = atomicAdd(&a.counts[b], n);
    __syncthreads();
    const int gb = s_base;
    for (int i = tid; i < n; i += 256) {
        const int idx = gb + i;
        if (idx >= 0 && idx < a.key_cap) gk[idx] = s_keys[i];     // (a counter that holds garbage cannot push a write outside the list)
    }
}

void launch_scan_decode(const PostArgs &a, int batch, hipStream_t s)
{
    const int per = scan_quads_per_block(a.A, a.nc);
    const size_t lds = (size_t)(per / 4) * a.nc * sizeof(unsigned long long);
    const int blocks = std::max(kScanBlocks, (a.A * 4 + per - 1) / per);
    launch_lds<scan_decode_kernel>(dim3(blocks, batch), dim3(256), lds, lds, s, a, per);
}
#endif   // IRMV_ALT_TU

// "IoU(a, b) > thr" as inter > thr * union (same expression as the oracle's iou_gt), the two areas handed in
// ((a[2] - a[0]) * (a[3] - a[1]), which a caller may compute once per box)
__device__ __forceinline__ bool iou_gt_area(const f32x4 a, float aa, const f32x4 b, float ab, float thr)
{
    const float ix1 = a[0] > b[0] ? a[0] : b[0];
    const float iy1 = a[1] > b[1] ? a[1] : b[1];
    const float ix2 = a[2] < b[2] ? a[2] : b[2];
    const float iy2 = a[3] < b[3] ? a[3] : b[3];
    float iw = ix2 - ix1, ih = iy2 - iy1;
    iw = iw > 0.0f ? iw : 0.0f;
    ih = ih > 0.0f ? ih : 0.0f;
    const float inter = iw * ih;
    const float uni = (aa + ab) - inter;
    return inter > thr * uni;
}
__device__ __forceinline__ bool iou_gt(const f32x4 a, const f32x4 b, float thr)
{
    return iou_gt_area(a, (a[2] - a[0]) * (a[3] - a[1]), b, (b[2] - b[0]) * (b[3] - b[1]), thr);
}

#ifndef IRMV_ALT_TU
__global__ void pnp_only_kernel(PnpConst c, const float *pts, int n, int armor_size, double *rvec, double *tvec, int32_t *ok)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    const bool good = solve_pnp_ippe(c, pts + 8 * i, armor_size, r, t, nullptr);
    for (int k = 0; k < 3; k++) { rvec[3 * i + k] = r[k]; tvec[3 * i + k] = t[k]; }
    ok[i] = good ? 1 : 0;
}

void launch_pnp_only(const PnpConst &c, const float *pts, int n, int armor_size, double *rvec, double *tvec, int32_t *ok, hipStream_t s)
{
    hipLaunchKernelGGL(pnp_only_kernel, dim3((n + 63) / 64), dim3(64), 0, s, c, pts, n, armor_size, rvec, tvec, ok);
}
#else
// irmv_pnp_solve2: both solutions of every quad, A first (mode MIN_ERR: nothing is picked)
__global__ void pnp_both_kernel(PnpConst c, const float *pts, int n, int armor_size, double *rvec, double *tvec, double *err, int32_t *ok)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0}, q[4];
    DevAlt alt;
    const PoseRule rule{kPoseMinErr, 1.0, 0.0, 0.0, 0.0, 0.0};
    const bool good = solve_pnp_ippe_both(c, pts + 8 * i, armor_size, r, t, q, rule, &alt);
    for (int k = 0; k < 3; k++) {
        rvec[6 * i + k] = r[k]; tvec[6 * i + k] = t[k];
        rvec[6 * i + 3 + k] = alt.rvec[k]; tvec[6 * i + 3 + k] = alt.tvec[k];
    }
    err[2 * i] = alt.err; err[2 * i + 1] = alt.err_alt;
    ok[i] = (good ? 1 : 0) | (alt.alt_ok ? 2 : 0);
}

void launch_pnp_both(const PnpConst &c, const float *pts, int n, int armor_size, double *rvec, double *tvec, double *err, int32_t *ok, hipStream_t s)
{
    hipLaunchKernelGGL(pnp_both_kernel, dim3((n + 63) / 64), dim3(64), 0, s, c, pts, n, armor_size, rvec, tvec, err, ok);
}
#endif   // IRMV_ALT_TU

// ---------------------------------------------------------------------------
// nms_pnp_kernel: one workgroup (1024 lanes = 16 waves) per frame, a sequence of phases, each a function below: take_keys,
// select_top_k (more keys than LDS holds), select_window (crowded frames, attempt 0), then the keys sorted (rank sort up to
// kRankSortUse keys: one pass, no barrier ladder; bitonic above that) and walked in score order by one of nms_class_walk,
// nms_full_matrix, nms_lazy_matrix, nms_class_lists; emit_records; store_records.
// The greedy walk is exactly the oracle's: same comparisons, same order.
// ---------------------------------------------------------------------------
constexpr int kRankSortMax = 2048;   // capacity of the rank-sort destination
constexpr int kRankSortUse = 512;    // above this the O(n^2) rank sort loses to the bitonic network
constexpr int kSupCap = 4096;   // candidates whose intra-block masks are precomputed
constexpr int kLazyN_ = 1024;   // most candidates of the lazy-matrix walk
// A crowded frame's first attempt works on the best kPreLo .. kPreHi candidates: <= 512 = the full-matrix walk, the fastest
// path there is (on the benchmark's frames the hundredth survivor sits among the first ~ 300 candidates)
constexpr int kPreHi = 512, kPreLo = 320;
constexpr int kMatW_ = 8;       // 64-bit words of a suppression-matrix row (512 candidates)
constexpr int kMatN = kMatW_ * 64;   // up to this many candidates the FULL suppression matrix fits ssup
constexpr int kLazyW = kLazyN_ / 64;
constexpr int kKptLds = 6144;   // class-walk path: the candidates' keypoint logits live in skeys[kKptLds ..) (16 KiB)
constexpr int kInScanU = 8;     // the in-kernel scan (no scan_decode_kernel in front): rounds of 1024 quads whose loads are issued together

// The kernel's small LDS variables.
struct NmsVars {
    int ncand, nanch;                        // take_keys: candidates / anchors with a candidate
    int digit, rem, fill;                    // the two radix selects
    int kept;                                // survivors of the walk
    int W;                                   // class walk: the widest class, in 64-bit words
    int cls_cnt[16];                         // nms_class_lists: kept candidates per class
    int cbase[16], ccnt[16];                 // class walk: first class-major position / size of every class
    unsigned int hist[256];                  // select_top_k
    unsigned long long keptw[kLazyW];        // per 64-candidate block: its survivors
    unsigned long long clsmask[16][kLazyW];  // per class and block: which candidates have that class (class_word_masks);
                                             // class walk, from its resolve on: row c = class c's survivors, class-local positions
};

// THE LDS MAP.  The arrays are declared in the kernel; every other use a phase makes of their bytes is a view below, named
// once, with who owns it and until when, and an assert that it fits.
struct NmsLds {
    unsigned long long *skeys;        // [kCandCap]      candidate keys (the bitonic network sorts them in place)
    unsigned long long *srank;        // [kRankSortMax]  rank-sort destination; select_window's compaction buffer
    unsigned long long *ssup;         // [kSupCap]       suppression masks / matrix rows, one 64-bit word per candidate and block
    f32x4 *stage_box;                 // [16][64]        nms_class_lists: per-wave block staging ...
    int *stage_cls;                   // [16][64]
    f32x4 *kept_box;                  // [kMaxDetCap]    the survivors, in score order
    int *kept_cls;
    unsigned long long *kept_key;
    unsigned short (*cls_list)[kMaxDetCap];   // [16]    nms_class_lists: per class, indices into kept_*
    NmsVars *v;

    static constexpr size_t kKeysBytes = kCandCap * sizeof(unsigned long long), kRankBytes = kRankSortMax * sizeof(unsigned long long),
                            kSupBytes = kSupCap * sizeof(unsigned long long), kStageSlots = 16 * 64;

    // ---- ssup before any mask is written (all of these end before the walk of their attempt builds its rows) ----
    // take_keys' in-kernel scan, until decode_boxes returns: the anchors that have a candidate, as 16-bit indices -- up to
    // 4 * kSupCap anchors (a 640 net has 8400); larger nets have no list and decode every anchor's box
    static_assert(4 * kSupCap * sizeof(unsigned short) <= kSupBytes && 4 * kSupCap <= 65536, "anchor list");
    __device__ __forceinline__ unsigned short *anchor_list(int A) const { return A <= 4 * kSupCap ? reinterpret_cast<unsigned short *>(ssup) : nullptr; }
    // select_window, per radix pass: [256 buckets][8 copies]
    static_assert(256 * 8 * sizeof(unsigned int) <= kSupBytes, "hist8");
    __device__ __forceinline__ unsigned int *hist8() const { return reinterpret_cast<unsigned int *>(ssup); }
    // rank_sort, from its first barrier to its last: one partial-rank counter per key
    static_assert(kRankSortUse * sizeof(int) <= kSupBytes, "rank counters");
    __device__ __forceinline__ int *rankacc() const { return reinterpret_cast<int *>(ssup); }
    // ---- ssup as matrix rows ----
    // nms_class_walk: [kRankSortUse rows][kMatW_ words][4 quarter words], read back as the 64-bit words they make up
    static_assert(kRankSortUse * kMatW_ * 4 * sizeof(unsigned short) <= kSupBytes, "rows16");
    __device__ __forceinline__ unsigned short *rows16() const { return reinterpret_cast<unsigned short *>(ssup); }
    // nms_full_matrix: [kMatN rows][kMatW_ words][2 halves]; nms_lazy_matrix: [64 rows][kLazyW words][2 halves] of the current block
    static_assert(kMatN * kMatW_ * 2 * sizeof(uint32_t) <= kSupBytes && 64 * kLazyW * 2 * sizeof(uint32_t) <= kSupBytes, "rows32");
    __device__ __forceinline__ uint32_t *rows32() const { return reinterpret_cast<uint32_t *>(ssup); }

    // ---- the staging as flat [1024] arrays: the three matrix-style walks, from their gather to the end of the attempt ----
    // boxes / classes of the candidates in score order (class -1: padding, or behind pre_nms_cap)
    static_assert(kLazyN_ <= kStageSlots, "cbox / ccls");
    __device__ __forceinline__ f32x4 *cbox() const { return stage_box; }
    __device__ __forceinline__ int *ccls() const { return stage_cls; }
    // nms_class_walk, behind its <= kRankSortUse candidates: boxes in class-major order / (score position << 8 | class)
    static_assert(2 * kRankSortUse <= kStageSlots, "mbox / minfo");
    __device__ __forceinline__ f32x4 *mbox() const { return stage_box + kRankSortUse; }
    __device__ __forceinline__ int *minfo() const { return stage_cls + kRankSortUse; }

    // nms_class_walk: box areas, class-major, behind the <= kRankSortUse sorted keys srank holds there
    static_assert(kRankSortUse * (sizeof(unsigned long long) + sizeof(float)) <= kRankBytes, "marea");
    __device__ __forceinline__ float *marea() const { return reinterpret_cast<float *>(srank + kRankSortUse); }

    // nms_class_walk -> emit_records: the candidates' keypoint logits in score order, 8 per candidate, in the tail of skeys
    // (the path has at most kRankSortUse keys, the rank sort's padding included, in front of them)
    static_assert(kRankSortUse <= kKptLds && kKptLds * sizeof(unsigned long long) + kRankSortUse * 8 * sizeof(float) <= kKeysBytes, "keypoint logits");
    __device__ __forceinline__ float *kpt_logits() const { return reinterpret_cast<float *>(skeys + kKptLds); }
    // nms_class_walk -> emit_records: survivor -> score position (the per-class lists are not used on that path)
    static_assert(kMaxDetCap * sizeof(unsigned short) <= sizeof(unsigned short[16][kMaxDetCap]), "kept_src");
    __device__ __forceinline__ unsigned short *kept_src() const { return cls_list[0]; }
    // emit_records -> store_records: the records' staging (the key list is dead: the survivors' keys sit in kept_key).  With
    // max_det > 236 it reaches into kpt_logits, which emit_records therefore reads first
    static_assert(sizeof(DevDet) % 16 == 0 && sizeof(DevDet) * kMaxDetCap <= kKeysBytes, "record staging");
    __device__ __forceinline__ DevDet *det_staging() const { return reinterpret_cast<DevDet *>(skeys); }
};

#define IRMV_STAMP(k) do { if (a.dbg && tid == 0) a.dbg[b * 16 + (k)] = clock64(); } while (0)

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- take keys.  Either scan_decode_kernel has filled the frame's key list and decoded the candidate anchors' boxes, or
// the scan runs here: class logits of every anchor -> candidate keys + the list of anchors that have one, then their boxes ----
__device__ __forceinline__ void take_keys(const PostArgs &a, const NmsLds &L, unsigned long long *gk, int b, int tid)
{
    if (a.counts) {
        // (a lane's first key is requested together with the count, not behind it: one memory round trip instead of two
        // for frames of up to 1024 candidates; beyond the count it is whatever the list holds, and is not used)
        // (round 4: ALL eight keys a lane can own in the LDS list are requested with the count -- a crowded frame's 2 000 .. 5 000
        // keys used to arrive in dependent round trips of 1024, one per loop iteration, ~ 1.5 us each on a single frame)
        constexpr int KPL = kCandCap / 1024;
        unsigned long long k_mine[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const int i = tid + k * 1024;
            k_mine[k] = gk[i < a.key_cap ? i : a.key_cap - 1];
        }
        int n = a.counts[b];
        n = n < 0 ? 0 : (n > a.key_cap ? a.key_cap : n);           // whatever the counter holds, reads stay inside the list
        if (n <= kCandCap) {
#pragma unroll
            for (int k = 0; k < KPL; k++)
                if (tid + k * 1024 < n) L.skeys[tid + k * 1024] = k_mine[k];
        }
        __syncthreads();                                           // every lane has read the count
        if (tid == 0) { L.v->ncand = n; a.counts[b] = 0; }         // the next step of this slot starts from zero
        if (a.cand_bits)                                           // ... and so does its candidate-anchor bitmap (sparse head)
            for (int i = tid; i < a.cand_words; i += blockDim.x) a.cand_bits[(size_t)b * a.cand_words + i] = 0u;
    } else {
        // Level by level (records of a level are contiguous), four lanes per anchor; the loads of U rounds are issued together.
        unsigned short *alist = L.anchor_list(a.A);
        constexpr int U = kInScanU;
        int lbase = 0;
        const float min_thr = a.cls->min_thr;   // class policy: the smallest per-class threshold (uniform: one scalar load)
#pragma unroll 1
        for (int l = 0; l < 3; l++) {
            const int lhw = (a.net_w / (8 << l)) * (a.net_h / (8 << l));
            const float *lrec = a.head_all + ((size_t)lbase * a.slots_total + (size_t)(a.first + b) * lhw) * kHeadRec;
            const int quads = lhw * 4;
            for (int q0 = 0; q0 < quads; q0 += 1024 * U) {
                f32x4 cl[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int t = q0 + u * 1024 + tid;
                    const int rin = t < quads ? (t >> 2) : 0;
                    cl[u] = reinterpret_cast<const f32x4 *>(lrec + (size_t)rin * kHeadRec + kClsOff)[tid & 3];
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (q0 + u * 1024 >= quads) break;          // workgroup-uniform
                    const int t = q0 + u * 1024 + tid;
                    scan_quad(a, min_thr, lbase + (t >> 2), t < quads, cl[u], L.skeys, gk, &L.v->ncand, alist, &L.v->nanch);
                }
            }
            lbase += lhw;
        }
        __syncthreads();
        decode_boxes(a, b, alist, alist ? L.v->nanch : a.A);   // boxes of the candidate anchors, in parallel over the whole workgroup
    }
}

// ---- More candidates than the LDS sort holds (noise frames): keep exactly the K = pre_nms_cap largest keys.  Keys are
// unique, so an 8-pass MSB-first radix select finds the K-th largest key T exactly; every key >= T is then compacted into
// LDS.  Same result as sorting everything and cutting at K.  Returns the number of keys in L.skeys ----
__device__ __forceinline__ int select_top_k(const PostArgs &a, const NmsLds &L, const unsigned long long *gk, int n_total, int tid)
{
    NmsVars &v = *L.v;
    const int K = a.pre_nms_cap < kCandCap ? a.pre_nms_cap : kCandCap;
    unsigned long long prefix = 0ull, mask = 0ull;
    if (tid == 0) { v.rem = K; v.fill = 0; }
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) v.hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n_total; i += blockDim.x) {
            const unsigned long long key = gk[i];
            if ((key & mask) == prefix) atomicAdd(&v.hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int rem = v.rem, d = 255;
            for (; d > 0; d--) {
                if ((int)v.hist[d] >= rem) break;
                rem -= (int)v.hist[d];
            }
            v.digit = d;
            v.rem = rem;
        }
        __syncthreads();
        prefix |= (unsigned long long)v.digit << shift;
        mask |= 0xffull << shift;
    }
    for (int i = tid; i < n_total; i += blockDim.x) {
        const unsigned long long key = gk[i];
        if (key >= prefix) {
            const int pos = atomicAdd(&v.fill, 1);
            if (pos < kCandCap) L.skeys[pos] = key;
        }
    }
    __syncthreads();
    return v.fill < kCandCap ? v.fill : kCandCap;
}

// ---- The best lo .. hi of the n_stored keys in L.skeys, compacted to its front: a radix threshold T with
// lo <= #{key >= T} <= hi.  MSB first, 8 bits per pass; a pass ends the search as soon as the buckets above the one that
// would overflow `hi` already hold `lo` keys (usually the first or second pass: any count in [lo, hi] will do, unlike the
// exact K-th key of select_top_k).  Returns the count ----
__device__ __forceinline__ int select_window(const NmsLds &L, int n_stored, int hi, int lo, int tid)
{
    NmsVars &v = *L.v;
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long prefix = 0ull, mask = 0ull, T = 0ull;
    int above = 0, m = 0;
    // eight copies of every bucket, picked by the lane: candidates all sit above the score threshold, so their keys
    // share their leading bits and a plain histogram's atomics pile onto two or three LDS words
    unsigned int *hist8 = L.hist8();
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < 256 * 8; i += blockDim.x) hist8[i] = 0u;
        __syncthreads();
        for (int i = tid; i < n_stored; i += blockDim.x) {
            const unsigned long long key = L.skeys[i];
            if ((key & mask) == prefix) atomicAdd(&hist8[(((unsigned)(key >> shift) & 255u) << 3) | (lane & 7)], 1u);
        }
        __syncthreads();
        if (wave == 0) {
            // lane L owns buckets 255 - 4 L .. 252 - 4 L; cumulative counts in descending bucket order
            const int d0 = 255 - 4 * lane;
            auto bucket = [&](int d) {
                const uint4 lo = *reinterpret_cast<const uint4 *>(&hist8[d << 3]), hi4 = *reinterpret_cast<const uint4 *>(&hist8[(d << 3) + 4]);
                return lo.x + lo.y + lo.z + lo.w + hi4.x + hi4.y + hi4.z + hi4.w;
            };
            const unsigned int h0 = bucket(d0), h1 = bucket(d0 - 1), h2 = bucket(d0 - 2), h3 = bucket(d0 - 3);
            const unsigned int tot = h0 + h1 + h2 + h3;
            unsigned int inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            const unsigned int exc = inc - tot + (unsigned int)above;
            const unsigned int c0 = exc + h0, c1 = c0 + h1, c2 = c1 + h2, c3 = c2 + h3;
            const unsigned long long cross = __ballot(c3 > (unsigned int)hi);
            if (cross == 0ull) {
                if (lane == 63) { v.digit = -1; v.rem = (int)c3; }             // everything under this prefix fits
            } else if (lane == __ffsll((long long)cross) - 1) {
                const int k = c0 > (unsigned int)hi ? 0 : (c1 > (unsigned int)hi ? 1 : (c2 > (unsigned int)hi ? 2 : 3));
                v.digit = d0 - k;                                              // the bucket that would overflow `hi`
                v.rem = (int)(k == 0 ? exc : (k == 1 ? c0 : (k == 2 ? c1 : c2)));   // keys above it
            }
        }
        __syncthreads();
        const int d = v.digit, before = v.rem;
        if (d < 0) { T = prefix; m = before; break; }
        if (before >= lo) { T = prefix | ((unsigned long long)(d + 1) << shift); m = before; break; }   // (d = 255 cannot get here: before = above < lo)
        prefix |= (unsigned long long)d << shift;
        mask |= 0xffull << shift;
        above = before;
        m = before;     // (after the last pass buckets are single keys: the loop has ended above)
    }
    if (tid == 0) v.fill = 0;
    __syncthreads();
    for (int i = tid; i < n_stored; i += blockDim.x) {
        const unsigned long long key = L.skeys[i];
        if (key >= T) {
            const int pos = atomicAdd(&v.fill, 1);
            if (pos < kRankSortMax) L.srank[pos] = key;
        }
    }
    __syncthreads();
    m = v.fill < hi ? v.fill : hi;                  // (= the count the search ended on)
    for (int i = tid; i < m; i += blockDim.x) L.skeys[i] = L.srank[i];
    __syncthreads();
    return m;
}

// ---- Boxes of the candidates whose keys sit in `keys[0 .. cnt)`, into the frame's global box list, four lanes per
// candidate (keys from the class-branch conv epilogues: nobody has decoded them yet; an anchor with several classes above
// threshold is decoded once per class: same value, same address).  Two rounds of 256 candidates per trip, both rounds' DFL
// logits requested before either is used (a store to the box list between them would otherwise order the second round's
// loads behind the first round's arithmetic) ----
__device__ __forceinline__ void decode_keys(const PostArgs &a, int b, const unsigned long long *keys, int cnt, int tid)
{
    const int q = tid & 3, lane = tid & 63;
    for (int i0 = 0; i0 < cnt; i0 += 512) {
        f32x4 v[2][4];
        int an_[2];
        bool live_[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int ci = i0 + u * 256 + (tid >> 2);
            live_[u] = ci < cnt;                               // quad-uniform
            an_[u] = live_[u] ? unpack_key(keys[ci], a.nc, a.A).an : 0;
            load_dfl(anchor_rec(a, b, an_[u]), q, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (i0 + u * 256 >= cnt) break;                    // workgroup-uniform
            const f32x4 box = box_from_dfl(v[u], an_[u], lane, a.net_w, a.net_h);
            if (live_[u] && q == 0) reinterpret_cast<f32x4 *>(a.boxes)[(size_t)b * a.A + an_[u]] = box;
        }
    }
}

// ---- Rank sort of n <= kRankSortUse keys, keys[] -> dst[] in descending order, for the whole workgroup.  Keys are unique,
// so "number of keys greater than mine" is a permutation.  A key's count is split over P lanes (all 1024 of the workgroup
// for n >= 342: with one lane per key a 380-candidate frame kept six waves busy for 16 k cycles), each counting over its
// own stretch of the list; the partial counts meet in a counter per key, acc[].  keys[] is padded to a multiple of 8 ----
__device__ __forceinline__ void rank_sort(unsigned long long *keys, int n, unsigned long long *dst, int *acc, int tid)
{
    const int n8 = (n + 7) & ~7;
    for (int i = n + tid; i < n8; i += blockDim.x) keys[i] = 0ull;   // pad: never greater than a real key
    for (int i = tid; i < n; i += blockDim.x) acc[i] = 0;
    __syncthreads();
    if (n > 0) {
        const int P = min(16, (int)blockDim.x / n);                         // lanes per key (n <= 512: at least two)
        const int per = ((n8 / 8 + P - 1) / P) * 8;                         // keys per stretch (a multiple of 8)
        const int p = tid / n, i = tid - p * n;
        const int j_lo = p * per, j_hi = min(j_lo + per, n8);
        if (p < P && j_lo < j_hi) {
            const unsigned long long mine = keys[i];
            int rank = 0;
#pragma unroll 2
            for (int j = j_lo; j < j_hi; j += 8) {
                const ulonglong2 k0 = *reinterpret_cast<const ulonglong2 *>(&keys[j]);
                const ulonglong2 k1 = *reinterpret_cast<const ulonglong2 *>(&keys[j + 2]);
                const ulonglong2 k2 = *reinterpret_cast<const ulonglong2 *>(&keys[j + 4]);
                const ulonglong2 k3 = *reinterpret_cast<const ulonglong2 *>(&keys[j + 6]);
                rank += (k0.x > mine) + (k0.y > mine) + (k1.x > mine) + (k1.y > mine) + (k2.x > mine) + (k2.y > mine) +
                        (k3.x > mine) + (k3.y > mine);
            }
            if (P == 1) acc[i] = rank; else atomicAdd(&acc[i], rank);
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) dst[acc[i]] = keys[i];
    __syncthreads();
}

// ---- The n_stored keys of L.skeys in descending order: rank sort into L.srank, or the bitonic network in place ----
__device__ __forceinline__ const unsigned long long *sort_keys(const NmsLds &L, int n_stored, int tid)
{
    if (n_stored <= kRankSortUse) {
        rank_sort(L.skeys, n_stored, L.srank, L.rankacc(), tid);
        return L.srank;
    }
    unsigned long long *skeys = L.skeys;
    int npow = 512;
    while (npow < n_stored) npow <<= 1;
    for (int i = n_stored + tid; i < npow; i += blockDim.x) skeys[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= npow; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npow; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = skeys[i], y = skeys[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) { skeys[i] = y; skeys[l] = x; }
                }
            }
            __syncthreads();
        }
    }
    return skeys;
}

// ===== steps the three matrix-style walks (class walk, full matrix, lazy matrix) share =====

// boxes (from the frame's global list) and classes of the first n sorted candidates into cbox / ccls, in score order, the
// classes padded with -1 (no class) up to the 64-candidate block boundary
__device__ __forceinline__ void gather_sorted(const PostArgs &a, const NmsLds &L, const unsigned long long *sorted, const f32x4 *boxes, int n, int tid)
{
    for (int i = tid; i < ((n + 63) & ~63); i += blockDim.x) {
        if (i < n) {
            const KeyId k = unpack_key(sorted[i], a.nc, a.A);
            L.cbox()[i] = boxes[k.an];
            L.ccls()[i] = k.cls;
        } else {
            L.ccls()[i] = -1;
        }
    }
}

// per class and 64-candidate word of the score order: which candidates have that class (one ballot per class and wave, waves
// 0 .. words - 1; nw = words that hold candidates) -- the class filter of a matrix row is then ONE 8-byte LDS read per word
// instead of sixteen 16-byte ones
__device__ __forceinline__ void class_word_masks(const NmsLds &L, int nw, int words, int nc, int lane, int wave)
{
    if (wave < words) {
        const int c = wave < nw ? L.ccls()[(wave << 6) + lane] : -1;
        for (int k = 0; k < nc; k++) {
            const unsigned long long mk = __ballot(c == k);
            if (lane == 0) L.v->clsmask[k][wave] = mk;
        }
    }
}

// Half h of word w of candidate i's suppression row: bit jj <=> candidate j = 64 w + 32 h + jj (j < i) has i's class and
// IoU(j, i) > thr -- who suppresses i if kept.  (An item is HALF a word: twice the items of half the length spread more
// evenly over the 1024 lanes -- a row's cost is its same-class candidates in the word, anything from none to 64.)
__device__ __forceinline__ uint32_t sup_row_half(const NmsLds &L, int i, int n, int w, int h, float iou_thr)
{
    uint32_t mask = 0u;
    const int j0 = (w << 6) + (h << 5);
    if (i < n && j0 < i) {
        const f32x4 bi = L.cbox()[i];
        const int ci = L.ccls()[i];
        const int jend = i - j0 < 32 ? i - j0 : 32;
        // class filter first (the per-class word of class_word_masks), then the IoU test only for the few same-class candidates
        uint32_t same = (uint32_t)(L.v->clsmask[ci][w] >> (h << 5));
        if (jend < 32) same &= (1u << jend) - 1u;
        while (same) {
            const int jj = __ffs((int)same) - 1;
            same &= same - 1u;
            if (iou_gt(L.cbox()[j0 + jj], bi, iou_thr)) mask |= 1u << jj;
        }
    }
    return mask;
}

// One wave resolves block blk of 64 candidates in order; lane's candidate has the suppression row `row` (64-bit words, one per
// block), keptw[w] = the survivors of earlier block w.  Returns the block's survivors.
// Without walking it candidate by candidate (one wave alone on its SIMD pays every instruction's full latency: ~200 cycles
// per survivor that way): a candidate whose possible suppressors (its sup bits) are all DECIDED is decided itself: kept iff
// none of them was kept.  Every round decides at least the first undecided candidate, usually most of them; the kept set is
// the sequential walk's.
__device__ __forceinline__ unsigned long long resolve_block(const unsigned long long *row, const unsigned long long *keptw, int blk, bool valid, int lane)
{
    bool alive = valid;
    for (int w = 0; w < blk; w++)                      // suppressed by a kept candidate of an earlier block?
        if (valid && (row[w] & keptw[w]) != 0ull) alive = false;
    const unsigned long long sup = valid ? row[blk] : 0ull;
    unsigned long long U = __ballot(alive), K = 0ull;   // undecided, kept
    while (U) {
        const bool ready = ((U >> lane) & 1ull) && (sup & U) == 0ull;
        const unsigned long long R = __ballot(ready);
        K |= __ballot(ready && (sup & K) == 0ull);
        U &= ~R;
    }
    return K;
}

// The cap on block blk's survivors K, `kept` survivors before it: the walk stops with the max_det-th survivor (a candidate's
// fate depends on the ones before it only).  Stores the accepted ones into kept_* and the block's word into keptw; returns
// the new count.
__device__ __forceinline__ int cap_and_keep(const NmsLds &L, const unsigned long long *sorted, unsigned long long K, int kept, int blk, int max_det, int lane)
{
    const int idx = (blk << 6) + lane;
    const int room = max_det - kept;
    unsigned long long A = K;
    if (__popcll(K) > room) {
        const bool over = ((K >> lane) & 1ull) && __popcll(K & ((1ull << lane) - 1ull)) >= room;
        A = K & ~__ballot(over);
    }
    const bool mine = (A >> lane) & 1ull;
    const int pos = kept + __popcll(A & ((1ull << lane) - 1ull));
    if (mine) {
        L.kept_box[pos] = L.cbox()[idx];
        L.kept_cls[pos] = L.ccls()[idx];
        L.kept_key[pos] = sorted[idx];
    }
    if (lane == 0) L.v->keptw[blk] = A;
    return kept + __popcll(A);
}

// ================= up to kRankSortUse candidates whose boxes nobody has decoded yet: the usual frame (round 4) =================
// Same algorithm, reorganised around three observations.  (1) A candidate's box is needed at its RANK, not at its anchor:
// the keys are sorted first, the boxes are decoded in score order straight into LDS and the keypoint logits come with
// them -- no store to and gather from the global box list (two memory round trips, ~ 2 us each on a lone frame), no
// keypoint read after the walk (a third).  (Requesting the logits BEFORE the sort, to run it under their round trip, was
// built first: 32 more registers across the sort loop spilled eighteen values to scratch memory all over the kernel.)  (2) Suppression is class-aware, so the walk of one class never looks at
// another: candidates are regrouped class-major (score order kept inside a class), the IoU tests of a row are then a
// DENSE run over the class's earlier members (no per-word class filter and bit loop: rows of different classes in one
// wave made every wave wait for its longest loop), and the sixteen waves walk the sixteen classes side by side.  (3) The
// max_det cap cuts the survivors in SCORE order whatever order they were found in: survivors are flagged at their
// score-order position and counted off there.  Comparisons, operands and their order are the oracle's: bit-identical
// (tests: every parity test runs this path; IRMV_NMS_CLASSWALK=0 is the round-3 path, compared bitwise).
// Returns the number of candidates walked.
__device__ __forceinline__ int nms_class_walk(const PostArgs &a, const NmsLds &L, int b, int n_stored)
{
    NmsVars &v = *L.v;
    f32x4 *cbox = L.cbox(), *mbox = L.mbox();
    int *ccls = L.ccls(), *minfo = L.minfo();
    float *marea = L.marea(), *ckpt = L.kpt_logits();
    unsigned long long *srank = L.srank, *ssup = L.ssup;
    // (lane numbers behind an opaque copy: the address arithmetic of this path, hoisted out of the attempt loop as loop
    // invariants, had seven values spilled to scratch memory at the loop's head and reloaded here)
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));
    const int tid = tid_, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = tid & 3;
    // ---- F1: rank sort ----
    if (tid < kLazyW) v.keptw[tid] = 0ull;
    rank_sort(L.skeys, n_stored, srank, L.rankacc(), tid);
    IRMV_STAMP(9);
    // ---- F2: boxes, classes and keypoints of the candidates IN SCORE ORDER: quad r / 4 decodes the candidate at sorted
    // position r.  Both rounds' logits are requested before either is used ----
    const int n = n_stored < a.pre_nms_cap ? n_stored : a.pre_nms_cap;
    {
        f32x4 dv[2][4];
        float kq0[2], kq1[2];
        KeyId id_[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int r = u * 256 + (tid >> 2);
            const bool live = r < n_stored;                    // quad-uniform
            id_[u] = unpack_key(live ? srank[r] : 0ull, a.nc, a.A);
            if (!live) id_[u].an = 0;
            const float *rec = anchor_rec(a, b, id_[u].an);
            load_dfl(rec, q, dv[u]);
            kq0[u] = a.nk >= 8 ? rec[kKptOff + 2 * q] : 0.f;
            kq1[u] = a.nk >= 8 ? rec[kKptOff + 2 * q + 1] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (u * 256 >= n_stored) break;                    // workgroup-uniform
            const int r = u * 256 + (tid >> 2);
            const f32x4 box = box_from_dfl(dv[u], id_[u].an, lane, a.net_w, a.net_h);
            if (r < n_stored) {
                if (q == 0) {
                    cbox[r] = box;
                    ccls[r] = r < n ? id_[u].cls : -1;   // (behind pre_nms_cap: not walked)
                }
                ckpt[8 * r + 2 * q] = kq0[u];
                ckpt[8 * r + 2 * q + 1] = kq1[u];
            }
        }
    }
    for (int i = n_stored + tid; i < ((n_stored + 63) & ~63); i += blockDim.x) ccls[i] = -1;   // padding up to the block boundary: no class
    __syncthreads();
    IRMV_STAMP(1);
    // ---- F4: class-major order ----
    const int nw = (n_stored + 63) >> 6;
    class_word_masks(L, nw, nw, a.nc, lane, wave);
    __syncthreads();
    if (wave == 0) {           // class sizes -> class-major base offsets, and the widest class in 64-bit words
        int cnt = 0;
        if (lane < a.nc)
            for (int w = 0; w < nw; w++) cnt += __popcll(v.clsmask[lane][w]);
        int inc = cnt, mx = cnt;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int t = __shfl_up(inc, o), m2 = __shfl_xor(mx, o);
            if (lane >= o) inc += t;
            mx = mx > m2 ? mx : m2;
        }
        if (lane < 16) { v.cbase[lane] = inc - cnt; v.ccnt[lane] = cnt; }
        if (lane == 0) v.W = (mx + 63) >> 6;
    }
    __syncthreads();
    if (tid < (nw << 6)) {
        const int i = tid, c = ccls[i];
        if (c >= 0) {
            int r = __popcll(v.clsmask[c][wave] & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; w++) r += __popcll(v.clsmask[c][w]);
            const int k = v.cbase[c] + r;
            const f32x4 box = cbox[i];
            mbox[k] = box;
            marea[k] = (box[2] - box[0]) * (box[3] - box[1]);
            minfo[k] = (i << 8) | c;
        }
    }
    __syncthreads();
    IRMV_STAMP(10);
    // ---- F5: suppression rows in CLASS-LOCAL coordinates: bit jj of word w of row k <=> member 64 w + jj of k's class
    // (earlier than k in score order) has IoU > thr with k.  An item is a quarter word (16 members); the quarter index is the
    // slowest-running one, so that whole waves fall idle where classes are shorter than the widest ----
    {
        const int W = v.W;
        unsigned short *rows16 = L.rows16();
        for (int item = tid; item < 4 * W * n; item += blockDim.x) {
            const int rest = item / n, k = item - rest * n;
            const int q4 = rest / W, w = rest - q4 * W;
            const int c = minfo[k] & 255, cb = v.cbase[c], r = k - cb;
            const int j0 = (w << 6) + (q4 << 4);
            unsigned int mask = 0u;
            if (j0 < r) {
                const f32x4 bi = mbox[k];
                const float ai = marea[k];
                const int jend = r - j0 < 16 ? r - j0 : 16;
                // all sixteen tests, predicated, in two batches of eight whose LDS reads are issued together: a loop to jend
                // paid the LDS latency and the test's dependent chain once per member (~ 300 cycles each).  (Members behind
                // jend: other rows of the list, or stale slots behind it inside the 512-slot arrays -- read, never used.)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if (8 * h >= jend) break;
                    f32x4 bj[8];
                    float aj[8];
#pragma unroll
                    for (int jj = 0; jj < 8; jj++) {
                        const int m = min(cb + j0 + 8 * h + jj, kRankSortUse - 1);
                        bj[jj] = mbox[m];
                        aj[jj] = marea[m];
                    }
#pragma unroll
                    for (int jj = 0; jj < 8; jj++)
                        if (8 * h + jj < jend && iou_gt_area(bj[jj], aj[jj], bi, ai, a.iou_thr)) mask |= 1u << (8 * h + jj);
                }
            }
            rows16[((k * kMatW_ + w) << 2) + q4] = (unsigned short)mask;
        }
    }
    __syncthreads();
    IRMV_STAMP(2);
    // ---- F6: wave c walks class c, 64 members per step ----
    if (wave < a.nc) {
        const int cnt = v.ccnt[wave], cb = v.cbase[wave];
        unsigned long long *ck = v.clsmask[wave];          // from here on: the class's survivors, class-local positions
        for (int blk = 0; blk < ((cnt + 63) >> 6); blk++) {
            const int il = (blk << 6) + lane, k = cb + il;
            const unsigned long long K = resolve_block(&ssup[k * kMatW_], ck, blk, il < cnt, lane);
            if (lane == 0) ck[blk] = K;
            if ((K >> lane) & 1ull) {
                const int i = minfo[k] >> 8;                 // flag the survivor at its score-order position
                atomicOr(reinterpret_cast<unsigned int *>(v.keptw) + (i >> 5), 1u << (i & 31));
            }
            wave_lds_sync();
        }
    }
    __syncthreads();
    // ---- F7: the first max_det survivors in score order ----
    if (tid < (nw << 6)) {
        const unsigned long long word = v.keptw[wave];
        if ((word >> lane) & 1ull) {
            int pos = __popcll(word & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; w++) pos += __popcll(v.keptw[w]);
            if (pos < a.max_det) {
                L.kept_box[pos] = cbox[tid];
                L.kept_cls[pos] = ccls[tid];
                L.kept_key[pos] = srank[tid];
                L.kept_src()[pos] = (unsigned short)tid;
            }
        }
    }
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < nw; w++) total += __popcll(v.keptw[w]);
        v.kept = total < a.max_det ? total : a.max_det;
    }
    return n;
}

// ---- up to kMatN candidates: the full suppression matrix.  Every IoU test the greedy walk can need, evaluated up front by
// the whole workgroup; the walk itself (wave 0, 64 candidates per step) is then AND / readlane work on 64-bit words (no boxes,
// no per-class kept lists).  Same comparisons as the oracle's walk ----
__device__ __forceinline__ void nms_full_matrix(const PostArgs &a, const NmsLds &L, const unsigned long long *sorted, const f32x4 *boxes, int b, int n, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    gather_sorted(a, L, sorted, boxes, n, tid);
    if (tid < kMatW_) L.v->keptw[tid] = 0ull;
    __syncthreads();
    const int nw = (n + 63) >> 6;
    class_word_masks(L, nw, kMatW_, a.nc, lane, wave);
    __syncthreads();
    IRMV_STAMP(10);
    // (consecutive lanes: consecutive i, same word -> broadcast reads of j)
    // (Measured and dropped: rows in two stages, the second only if the walk over the first has not filled max_det -- on
    // the 380-candidate benchmark frame the hundredth survivor sits in the fifth of six blocks, and the extra barriers cost
    // more than the unbuilt rows save.)
    uint32_t *rows32 = L.rows32();
    for (int item = tid; item < 2 * n * nw; item += blockDim.x) {
        const int h = item & 1, it2 = item >> 1;
        const int w = it2 / n, i = it2 - w * n;
        rows32[(i * kMatW_ + w) * 2 + h] = sup_row_half(L, i, n, w, h, a.iou_thr);
    }
    __syncthreads();
    IRMV_STAMP(2);
    if (wave == 0) {
        int kept = 0;
        for (int blk = 0; blk < nw && kept < a.max_det; blk++) {
            const int idx = (blk << 6) + lane;
            const unsigned long long K = resolve_block(&L.ssup[idx * kMatW_], L.v->keptw, blk, idx < n, lane);
            kept = cap_and_keep(L, sorted, K, kept, blk, a.max_det, lane);
            wave_lds_sync();
        }
        if (lane == 0) L.v->kept = kept;
    }
}

// ---- crowded frames (kMatN + 1 .. kLazyN_ candidates): the same matrix rows, built one 64-candidate block at a time
// right before the walk reaches that block, and not at all once max_det survivors are found.  (A frame with 900
// candidates fills max_det = 100 in its first few hundred; the all-pairs matrix would run 6 x the IoU tests of a
// 380-candidate frame, and the per-class-list walk took 85 us on such frames.) ----
__device__ __forceinline__ void nms_lazy_matrix(const PostArgs &a, const NmsLds &L, const unsigned long long *sorted, const f32x4 *boxes, int b, int n, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    gather_sorted(a, L, sorted, boxes, n, tid);
    if (tid < kLazyW) L.v->keptw[tid] = 0ull;
    if (tid == 0) L.v->kept = 0;
    __syncthreads();
    const int nw = (n + 63) >> 6;
    class_word_masks(L, nw, kLazyW, a.nc, lane, wave);        // 16 waves = 16 blocks of 64
    __syncthreads();
    uint32_t *rows32 = L.rows32();
    IRMV_STAMP(2);
    for (int blk = 0; blk < nw; blk++) {
        if (L.v->kept >= a.max_det) break;                     // workgroup-uniform (read behind the barrier below)
        for (int item = tid; item < 128 * (blk + 1); item += blockDim.x) {
            const int h = item & 1, row = (item >> 1) & 63, w = item >> 7;
            rows32[(row * kLazyW + w) * 2 + h] = sup_row_half(L, (blk << 6) + row, n, w, h, a.iou_thr);
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned long long K = resolve_block(&L.ssup[lane * kLazyW], L.v->keptw, blk, (blk << 6) + lane < n, lane);
            const int kept = cap_and_keep(L, sorted, K, L.v->kept, blk, a.max_det, lane);
            if (lane == 0) L.v->kept = kept;
        }
        __syncthreads();
    }
}

// "who of the 64 candidates of my block suppresses me": bit j set iff j < lane, same class, IoU > thr.
// sbox / scls: this wave's private LDS staging of the block.
__device__ __forceinline__ unsigned long long block_sup_mask(f32x4 box, int cls, int lane, float iou_thr, f32x4 *sbox, int *scls)
{
    sbox[lane] = box;
    scls[lane] = cls;
    wave_lds_sync();
    unsigned long long sup = 0ull;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
        const f32x4 bj = sbox[j];
        const int cj = scls[j];
        if (j < lane && cj == cls && cls >= 0 && iou_gt(bj, box, iou_thr)) sup |= 1ull << j;
    }
    wave_lds_sync();
    return sup;
}

// ---- any number of candidates.  All 16 waves, one 64-candidate block each: the block's 64x64 same-class IoU > thr relation
// as one 64-bit "who suppresses me" mask per candidate (independent of the kept set, so it is computed up front, in parallel,
// for the first kSupCap).  Wave 0 then walks the blocks in score order: test against the kept boxes OF THE CANDIDATE'S CLASS
// (per-class kept lists), resolve the block with ballots, append survivors ----
__device__ __forceinline__ void nms_class_lists(const PostArgs &a, const NmsLds &L, const unsigned long long *sorted, const f32x4 *boxes, int b, int n, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int n_pre = n < kSupCap ? n : kSupCap;
    for (int start = wave * 64; start < n_pre; start += 16 * 64) {
        const int idx = start + lane;
        const bool valid = idx < n;
        const KeyId k = unpack_key(valid ? sorted[idx] : 0ull, a.nc, a.A);
        const f32x4 box = valid ? boxes[k.an] : (f32x4){0.f, 0.f, 0.f, 0.f};
        L.ssup[idx] = block_sup_mask(box, valid ? k.cls : -1, lane, a.iou_thr, L.stage_box + 64 * wave, L.stage_cls + 64 * wave);
    }
    __syncthreads();
    IRMV_STAMP(2);
    if (wave == 0) {
        int kept = 0;
        for (int start = 0; start < n && kept < a.max_det; start += 64) {
            const int idx = start + lane;
            const bool valid = idx < n;
            const unsigned long long key = valid ? sorted[idx] : 0ull;
            const KeyId kid = unpack_key(key, a.nc, a.A);
            const int cls = valid ? kid.cls : -1;
            const f32x4 box = valid ? boxes[kid.an] : (f32x4){0.f, 0.f, 0.f, 0.f};
            // against the kept boxes of my class
            bool alive = valid;
            const int mycnt = valid ? L.v->cls_cnt[cls] : 0;
            for (int j = 0; __any(j < mycnt); j++) {
                if (j < mycnt) {
                    const int k = L.cls_list[cls][j];
                    if (iou_gt(L.kept_box[k], box, a.iou_thr)) alive = false;
                }
            }
            const unsigned long long sup = start < n_pre ? L.ssup[idx]
                                                        : block_sup_mask(box, cls, lane, a.iou_thr, L.stage_box, L.stage_cls);
            // sequential resolve, earliest first
            unsigned long long A = __ballot(alive);
            int taken = 0;
            for (unsigned long long todo = A; todo;) {          // walk the still-alive candidates in order
                const int j = __ffsll((long long)todo) - 1;
                if (kept + taken >= a.max_det) {
                    A &= (1ull << j) - 1ull;                      // cap reached: drop j and everything after
                    break;
                }
                taken++;
                const unsigned long long col = __ballot((sup >> j) & 1ull);   // lanes that j suppresses (all > j)
                A &= ~col;
                todo = A & ~((2ull << j) - 1ull);
            }
            const bool mine = (A >> lane) & 1ull;
            const int pos = kept + __popcll(A & ((1ull << lane) - 1ull));
            if (mine) {
                L.kept_box[pos] = box;
                L.kept_cls[pos] = cls;
                L.kept_key[pos] = key;
            }
            if (mine) L.cls_list[cls][atomicAdd(&L.v->cls_cnt[cls], 1)] = (unsigned short)pos;   // order within a class is irrelevant
            wave_lds_sync();
            kept += __popcll(A);
        }
        if (lane == 0) L.v->kept = kept;
    }
}

// ---- one PAIR of lanes per survivor: the record is assembled redundantly on both lanes, the fp64 PnP runs spread over them
// (solve_pnp_ippe_pair: two undistorted points / one IPPE solution per lane), lane 0 stages the record in LDS.
// kAlt: solve with solve_pnp_ippe_pair_both -- the prior may report B -- and the pair's odd lane stores the survivor's DevAlt ----
template <bool kAlt>
__device__ __forceinline__ void emit_records(const PostArgs &a, const NmsLds &L, int b, int kept, bool kp_lds, int tid)
{
    const int j = tid >> 1;
    // keypoint logits: from LDS where the class-walk path has put them, else from the head record.  (Read BEFORE the
    // staging is written: see det_staging.)
    float kpv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int an = 0;
    if (j < kept) {
        an = unpack_key(L.kept_key[j], a.nc, a.A).an;
        if (kp_lds) {
            const f32x4 *kl = reinterpret_cast<const f32x4 *>(L.kpt_logits() + 8 * L.kept_src()[j]);
            const f32x4 k0 = kl[0], k1 = kl[1];
            kpv[0] = k0[0]; kpv[1] = k0[1]; kpv[2] = k0[2]; kpv[3] = k0[3];
            kpv[4] = k1[0]; kpv[5] = k1[1]; kpv[6] = k1[2]; kpv[7] = k1[3];
        } else {
            const float *kp = anchor_rec(a, b, an) + kKptOff;
#pragma unroll
            for (int q = 0; q < 8; q++) kpv[q] = q < a.nk ? kp[q] : 0.f;
        }
    }
    __syncthreads();
    if (kept == 0) { IRMV_STAMP(11); IRMV_STAMP(12); }   // (diagnostic stamps: a frame without survivors has no keypoint / PnP phase; without these its two slots printed garbage)
    if (j < kept) {           // pair-uniform
        // the record's fields go to the LDS staging as they are produced (lane 0 of the pair): held in registers across the
        // solver they spilled
        DevDet *d = &L.det_staging()[j];
        const bool w = (tid & 1) == 0;
        const f32x4 box = L.kept_box[j];
        const unsigned long long key = L.kept_key[j];
        const float logit = unorderable((uint32_t)(key >> 32));
        int ix, iy, s, lbase, lhw, rin;
        anchor_geom(an, a.net_w, a.net_h, ix, iy, s, lbase, lhw, rin);
        const float axm = ((float)ix + 0.5f) - 0.5f, aym = ((float)iy + 0.5f) - 0.5f, sf = (float)s;
        if (w) {
            d->score = 1.0f / (1.0f + irmv_expf(-logit));
            d->cls = L.kept_cls[j];
            d->anchor = an;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                d->box_net[i] = box[i];
                const float off = (i & 1) ? a.off_y : a.off_x, sc = (i & 1) ? a.scale_y : a.scale_x;
                d->xyxy[i] = (box[i] - off) * sc;
            }
        }
        float px0 = 0.f, py0 = 0.f, px1 = 0.f, py1 = 0.f;      // this lane's two points for the solver (q and q + 2)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float kx = 0.f, ky = 0.f;
            if (2 * q + 1 < a.nk) {
                kx = (2.0f * kpv[2 * q] + axm) * sf;
                ky = (2.0f * kpv[2 * q + 1] + aym) * sf;
            }
            const float sx = (kx - a.off_x) * a.scale_x, sy = (ky - a.off_y) * a.scale_y;
            if ((q & 1) == (tid & 1)) {
                if (q < 2) { px0 = sx; py0 = sy; } else { px1 = sx; py1 = sy; }
            }
            if (w) {
                d->kpts_net[2 * q] = kx;
                d->kpts_net[2 * q + 1] = ky;
                d->kpts[2 * q] = sx;
                d->kpts[2 * q + 1] = sy;
            }
        }
        IRMV_STAMP(11);
        double rvec[3] = {0.0, 0.0, 0.0}, tvec[3] = {0.0, 0.0, 0.0}, quat[4] = {0.0, 0.0, 0.0, 1.0};
        int pnp_ok = 0;
        const int plate = a.cls->plate[L.kept_cls[j] & (kMaxClasses - 1)];   // class policy: the object points of this detection's class
        if constexpr (kAlt) {
            DevAlt alt{};
            if (a.nk >= 8) {
                const PoseRule rule = pose_rule(a.prior, a.up + 3 * (size_t)(a.first + b), L.kept_cls[j]);
                pnp_ok = solve_pnp_ippe_pair_both(a.pnp[(size_t)(a.first + b) * a.pnp_stride], px0, py0, px1, py1, plate, rvec, tvec, quat, rule, &alt) ? 1 : 0;
            }
            if (!w) a.alts[(size_t)b * a.max_det + j] = alt;   // (the pair's other lane stages the record)
        } else {
            if (a.nk >= 8) pnp_ok = solve_pnp_ippe_pair(a.pnp[(size_t)(a.first + b) * a.pnp_stride], px0, py0, px1, py1, plate, rvec, tvec, quat) ? 1 : 0;
        }
        IRMV_STAMP(12);
        if (w) {
#pragma unroll
            for (int i = 0; i < 3; i++) { d->rvec[i] = rvec[i]; d->tvec[i] = tvec[i]; }
#pragma unroll
            for (int i = 0; i < 4; i++) d->quat[i] = quat[i];
            d->pnp_ok = pnp_ok;
            d->armor_valid = a.nk >= 8 ? 1 : 0;   // keypoint head: every detection carries its four points
            d->armor_size = plate;
            d->n_lights = 0;
            d->pad_ = 0;
        }
    }
}

// ---- The frame's records leave as ONE contiguous run of 16-byte stores (13 per record), zero-padded behind the last
// survivor as EfficientNMS pads its outputs.  (One lane per record storing its own 208
// bytes put 16 different cache lines under every store instruction: 4 us of a 38 us frame went into that.) ----
__device__ __forceinline__ void store_records(const PostArgs &a, const NmsLds &L, int b, int kept, int tid)
{
    constexpr int kVec = sizeof(DevDet) / 16;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(L.det_staging());
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.dets + (size_t)b * a.max_det);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int i = tid; i < a.max_det * kVec; i += blockDim.x) dst[i] = i < kept * kVec ? src[i] : zero;
}

// kAlt (engines after their first irmv_engine_set_pose_prior): see emit_records.  kAlt = false is the kernel as it has always been.
template <bool kAlt>
__global__ __launch_bounds__(1024) void nms_pnp_kernel(PostArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned long long skeys[kCandCap];   // 64 KiB
    __shared__ unsigned long long srank[kRankSortMax];      // 16 KiB
    __shared__ __attribute__((aligned(16))) unsigned long long ssup[kSupCap];   // 32 KiB
    __shared__ f32x4 stage_box[16][64];                     // 16 KiB
    __shared__ __attribute__((aligned(16))) int stage_cls[16][64];   // (16-byte aligned: the matrix phase reads it as int4)
    __shared__ f32x4 kept_box[kMaxDetCap];
    __shared__ int kept_cls[kMaxDetCap];
    __shared__ unsigned long long kept_key[kMaxDetCap];
    __shared__ unsigned short cls_list[16][kMaxDetCap];
    __shared__ NmsVars sv;
    static_assert(sizeof(skeys) == NmsLds::kKeysBytes && sizeof(srank) == NmsLds::kRankBytes && sizeof(ssup) == NmsLds::kSupBytes &&
                  sizeof(stage_box) == NmsLds::kStageSlots * sizeof(f32x4) && sizeof(stage_cls) == NmsLds::kStageSlots * sizeof(int), "the LDS map's extents");
    const NmsLds L{skeys, srank, ssup, &stage_box[0][0], &stage_cls[0][0], kept_box, kept_cls, kept_key, cls_list, &sv};

    const int b = blockIdx.x, tid = threadIdx.x;
    IRMV_STAMP(0);
    unsigned long long *gk = a.keys + (size_t)b * a.key_cap;
    if (tid < 16) sv.cls_cnt[tid] = 0;
    if (tid == 0) { sv.ncand = 0; sv.nanch = 0; }
    __syncthreads();
    take_keys(a, L, gk, b, tid);
    __syncthreads();   // keys in LDS / global and boxes in global are visible to the whole workgroup from here
    IRMV_STAMP(7);
    const int n_total = sv.ncand;
    // The greedy walk visits candidates in score order and stops at max_det survivors, so on a crowded frame only the head
    // of the sorted list is ever looked at.  ATTEMPT 0 therefore works on the frame's best <= kPreHi candidates only (an
    // exact radix threshold: every key >= T, and nothing else): select, decode THEIR boxes, sort, walk.  If that walk
    // fills max_det -- or has seen everything the full algorithm would (pre_nms_cap <= the selected count) -- it IS the
    // full algorithm's result: a candidate's fate depends only on the candidates before it.  Otherwise (rare: few
    // survivors among the first thousand candidates) ATTEMPT 1 runs the whole list, as before.  A frame of 4 900 candidates
    // decodes, sorts and masks a fifth of them: the NMS kernel's 0.24 ms on such frames was all tail.
    const int pre_hi = a.prefilter > 1 ? (a.prefilter & 0xffff) : kPreHi, pre_lo = a.prefilter > 1 ? (a.prefilter >> 16) : kPreLo;   // (> 1: experiment override, hi | lo << 16)
    const bool prefilter_on = a.prefilter != 0 && n_total > pre_hi;
    bool kp_lds = false;                                  // the survivors' keypoint logits sit in LDS (class-walk path)
    for (int attempt = prefilter_on ? 0 : 1; attempt < 2; attempt++) {
        int n_stored = n_total, n;
        if (attempt == 1 && prefilter_on) {            // start over on the whole list
            if (tid < 16) sv.cls_cnt[tid] = 0;
            if (n_total <= kCandCap)
                for (int i = tid; i < n_total; i += blockDim.x) skeys[i] = gk[i];
            __syncthreads();
        }
        if (n_total > kCandCap) n_stored = select_top_k(a, L, gk, n_total, tid);
        const int n_full = n_stored < a.pre_nms_cap ? n_stored : a.pre_nms_cap;   // candidates the full algorithm walks
        bool truncated = false;
        if (attempt == 0) {
            n_stored = select_window(L, n_stored, pre_hi, pre_lo, tid);
            truncated = true;
        }
        IRMV_STAMP(8);
        kp_lds = a.keys_only && a.classwalk && n_stored <= kRankSortUse;
        if (kp_lds) {
            n = nms_class_walk(a, L, b, n_stored);
        } else {
            if (a.keys_only) {
                decode_keys(a, b, skeys, n_stored, tid);
                __syncthreads();                                // boxes visible to the whole workgroup
            }
            IRMV_STAMP(9);
            const unsigned long long *sorted = sort_keys(L, n_stored, tid);
            n = n_stored < a.pre_nms_cap ? n_stored : a.pre_nms_cap;
            const f32x4 *boxes = reinterpret_cast<const f32x4 *>(a.boxes) + (size_t)b * a.A;
            IRMV_STAMP(1);
            if (n <= kMatN) nms_full_matrix(a, L, sorted, boxes, b, n, tid);
            else if (n <= kLazyN_) nms_lazy_matrix(a, L, sorted, boxes, b, n, tid);
            else nms_class_lists(a, L, sorted, boxes, b, n, tid);
        }
        __syncthreads();
        // attempt 0 stands if it filled max_det or walked everything the full algorithm would walk
        if (!truncated || sv.kept >= a.max_det || n >= n_full) break;
        __syncthreads();                                    // (everyone has read the count before the next attempt resets it)
    }
    IRMV_STAMP(3);
    const int kept = sv.kept;
    if (tid == 0) {
        a.fout[b] = DevFrameOut{kept, n_total, 0, 0};   // (overflow: the candidate list is sized for every (anchor, class) pair; kept for ABI stability)
    }
    emit_records<kAlt>(a, L, b, kept, kp_lds, tid);
    __syncthreads();
    store_records(a, L, b, kept, tid);
    IRMV_STAMP(4);
    if (a.dbg && tid == 0) { a.dbg[b * 16 + 5] = n_total; a.dbg[b * 16 + 6] = kept; }
}
#undef IRMV_STAMP

#ifdef IRMV_ALT_TU
void launch_nms_pnp_alt(const PostArgs &a, int batch, hipStream_t s)
{
    hipLaunchKernelGGL(nms_pnp_kernel<true>, dim3(batch), dim3(1024), 0, s, a);
}
#else
void launch_nms_pnp(const PostArgs &a, int batch, hipStream_t s)
{
    if (a.alts) launch_nms_pnp_alt(a, batch, s);
    else hipLaunchKernelGGL(nms_pnp_kernel<false>, dim3(batch), dim3(1024), 0, s, a);
}

// The candidate counts the kernels above branch on, as compiled (irmv_post_limits: tests/post_ladder.py builds its count
// ladders from them, so a threshold that moves takes its tests along).
void post_limits(int32_t out[16])
{
    const int32_t v[16] = {kRankSortUse, kRankSortMax, kLazyN_, kSupCap, kCandCap, kPreHi, kPreLo, kMaxTiles, kMaxDetCap,
                           kScanBlocks, 256 * kScanU, (int32_t)kScanLdsMax, 1024 * kInScanU, kMatW_ * 64, 0, 0};
    for (int i = 0; i < 16; i++) out[i] = v[i];
}
#endif   // IRMV_ALT_TU

}  // namespace irmv
