// The box branch of one Detect level -- 3x3 (Cin -> 64), 3x3 (64 -> 64), 1x1 (64 -> 64) -- at the step's CANDIDATE ANCHORS only,
// and, where the plan links the two (BoxGatherArgs::kw0), the level's keypoint branch -- 3x3 (Cin -> 16), 3x3 (16 -> 16), 1x1
// (16 -> nk) -- at the same anchors in the same launch.
//
// nms_pnp_kernel reads a box row only at a candidate anchor, and the benchmark's frames have 184 of 8 400 (2.2 %).  The tile
// gate of the layer kernels (k_conv.hip) cannot follow that far down: a tile of the 40 x 40 and 20 x 20 maps is too coarse,
// and a workgroup keeps its tile position over many images.  Here the work is a compact list instead:
//
//   cand_list_kernel   one workgroup per image turns the candidate bitmap the class carriers have set into the image's list
//                      of candidate pixels per level (LDS counters; the order inside an image is whatever the atomics give
//                      -- every row is computed on its own, no stored bit depends on it)
//   box_gather_kernel  a fixed grid of persistent workgroups.  Every workgroup scans the per-image counts into a prefix, so
//                      candidate k of the level is (image, entry) by a binary search, and takes the passes p = blockIdx,
//                      blockIdx + grid, ... of 2 x 16 candidates: an equal share for every workgroup whatever the frames hold.
//                      Workgroups without a pass return behind the scan, before they stage anything.
//
// A pass: two groups of three waves, each group on 16 candidates = one MFMA column tile.
//   stage 1   cv2.L.0 at the 3 x 3 pixels around each candidate (wave w: the row y - 1 + w, three column tiles x four
//             16-channel tiles); the 3 x 5 input pixels a wave needs per 32-channel chunk come straight from memory as B
//             fragments (the rows of a 5 x 5 neighbourhood are cache hits between the waves), loaded in a lane mapping that
//             puts four consecutive lanes on one 64-byte piece and moved to the MFMA's lanes by ds_bpermute_b32 (to_mfma_lanes
//             below: the gathered input lines, not the MFMAs, are what a slab step waits for); SiLU, fp16, into an LDS plane
//             [position][candidate][64 channels] -- ZERO where the position lies outside the map (the second conv's padding)
//   stage 2   cv2.L.1 at the candidates out of that plane (the group's first wave), SiLU, fp16, into the plane's first rows
//   final     the 1x1 (the group's second wave, behind a barrier: its B fragments are LDS reads, so no MFMA of this file
//             reads a register that inline asm wrote and no mfma_operand_fence is needed), * ln 2 + bias, four f32x4 stores
//             per lane into the head row's box channels
//   keypoints a fourth wave per group (the KPT instantiations: 512 threads) computes cv4.L.0 at the nine positions from the whole
//             5 x 5 neighbourhood, cv4.L.1 and the final at the candidate, on a plane of its own -- kpt3_kernel's operands,
//             K order and roundings (k_kpt.hip); it joins the pass's barriers and adds none.  Launch names stay box_gather_c*.
// Weights: the nt = 4 packing of the LDS family, one 36 KiB chunk slab at a time through LDS for both groups, two buffers:
// the next slab travels in registers under the current one's MFMAs and is written beside it, one barrier per slab.  A pass is
// a chain of Cin / 32 + 2 such slab steps, and a launch lasts as long as the longest chain of passes: that, not the MFMA
// count, is what its time follows.
//
// The bit contract: per output element the instruction (v_mfma_f32_16x16x32_f16), the operands and the K order of
// conv3x3_lds_body -- accumulators start at the bias, chunks of 32 channels outermost, the nine taps inside, taps that leave
// the map run with zero operands (a skipped MFMA changes a -0), silu_pack8 between the stages, the N2 = 4 epilogue's
// arithmetic for the final.  A column of an MFMA does not depend on its neighbours, so which pixels share a tile is free.
#include "irmv_common.hpp"

namespace irmv {

namespace {
constexpr int GNG = 2;                    // candidate groups per pass
constexpr int GNT = GNG * 192;            // three waves per group: the box branch's, and the threads that stage the weight slabs
constexpr int GNTK = GNG * 256;           // ... with the keypoint branch on board: a fourth wave per group (it stages nothing)
constexpr int GSLAB = 9 * 4 * 64;         // half8 of a chunk slab: [tap][tile][lane], 36 KiB
constexpr int GWPT = GSLAB / GNT;         // ... per thread
constexpr int GROW = 16 * 128;            // bytes of a position of the plane: [candidate][64 channels]
constexpr int GMID = 9 * GROW;            // bytes of a group's plane
constexpr int GMAXB = 1024;               // images of a launch (the prefix lives in LDS)
constexpr size_t GWLDS = (size_t)2 * GSLAB * 16;   // two chunk slabs of weights: the MFMAs run on one while the next is written
constexpr size_t GLDS = GWLDS + (size_t)GNG * GMID + (size_t)GMAXB * 4;
constexpr int KROW = 16 * 32;             // bytes of a position of the keypoint plane: [candidate][16 channels]
constexpr int KMID = 10 * KROW;           // bytes of a group's keypoint plane: the nine positions, then the second conv's activated sums
constexpr size_t GLDSK = GLDS + (size_t)GNG * KMID;
static_assert(GSLAB % GNT == 0, "every thread stages the same number of slab pieces");
static_assert(GLDSK <= 160 * 1024, "a CU's LDS");   // (ONE workgroup per CU, by the register file too: 240 - 251 VGPRs, no scratch; bounded to 168 the stage-1 waves spill)
}  // namespace

__global__ __launch_bounds__(256) void cand_list_kernel(CandListArgs a)
{
    __shared__ int s_n[3];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) s_n[tid] = 0;
    __syncthreads();
    const int A = a.abase[2] + a.hw[2];
    for (int wd = tid; wd < a.cand_words; wd += 256) {
        unsigned int w = a.cand_bits[(size_t)img * a.cand_words + wd];
        while (w) {
            const int an = wd * 32 + __builtin_ctz(w);
            w &= w - 1u;
            const int lv = an >= a.abase[2] ? 2 : (an >= a.abase[1] ? 1 : 0);
            if (an < A && a.list[lv]) a.list[lv][(size_t)img * a.hw[lv] + atomicAdd(&s_n[lv], 1)] = an - a.abase[lv];   // (an anchor has one bit: the count stays below hw)
        }
    }
    __syncthreads();
    if (tid < 3 && a.count[tid]) a.count[tid][img] = s_n[tid];
}

void launch_cand_list(const CandListArgs &a, int batch, hipStream_t s)
{
    hipLaunchKernelGGL(cand_list_kernel, dim3(batch), dim3(256), 0, s, a);
}

// STEPS = Cin / 64 (1, 2, 4); KPT: the level's keypoint branch rides along (BoxGatherArgs::kw0), on a fourth wave per group
template <int STEPS, bool KPT>
__global__ __launch_bounds__(KPT ? GNTK : GNT) void box_gather_kernel(BoxGatherArgs a, int batch)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    half8 *s_w2 = reinterpret_cast<half8 *>(smem);                // two chunk slabs of weights: slab k of a pass in buffer k & 1 (a pass has an even number)
    uint8_t *s_mid = smem + GWLDS;                                // the groups' planes
    int *s_pre = reinterpret_cast<int *>(smem + GWLDS + (size_t)GNG * GMID);   // inclusive prefix of the images' counts
    constexpr int CH1 = 2 * STEPS, NCH = CH1 + 2;                 // chunk slabs of a pass: the first conv's, then the second conv's two
    constexpr int NW = KPT ? 4 : 3;                               // waves of a group
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = wave / NW, row = wave - sub * NW;
    const int tid = (int)threadIdx.x - (KPT ? sub * 64 : 0);   // the box waves' index among themselves: GNT threads stage the slabs
    const int g = lane >> 4, r = lane & 15;
    const int H = a.H, W = a.W, HW = H * W;

    // ---- the list: candidate k of the level is entry k - pre[img - 1] of the first image whose prefix exceeds k ----
    if (wave == 0) {
        int carry = 0;
        for (int base = 0; base < batch; base += 64) {
            const int i = base + lane;
            int v = i < batch ? min(max(a.count[i], 0), HW) : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(v, d);
                if (lane >= d) v += t;
            }
            v += carry;
            if (i < batch) s_pre[i] = v;
            carry = __shfl(v, 63);
        }
    }
    __syncthreads();
    const int n = s_pre[batch - 1];
    if ((int)blockIdx.x * (GNG * 16) >= n) return;   // (the whole workgroup, before it stages anything)

    const int img_stride = HW * a.x_ld * 2;
    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t *>(a.x), 0, batch * img_stride, 0x00020000);
    const half8 *w0 = reinterpret_cast<const half8 *>(a.w0), *w1 = reinterpret_cast<const half8 *>(a.w1);
    half8 rw[GWPT];
    auto fetch_slab = [&](int k) {
        const half8 *src = k < CH1 ? w0 + (size_t)k * GSLAB : w1 + (size_t)(k - CH1) * GSLAB;
#pragma unroll
        for (int i = 0; i < GWPT; i++) rw[i] = src[tid + i * GNT];
    };
    // slab k -> its LDS buffer, slab k + 1 (the next pass's first behind the last) -> registers, under slab k's MFMAs.  ONE
    // barrier per slab: the buffer written here was last read by the MFMAs of slab k - 2, and every wave has passed the
    // barrier of slab k - 1 since.
    static_assert(NCH % 2 == 0, "slab k of every pass lies in buffer k & 1");
    auto stage_slab = [&](int k) {
        half8 *s_w = s_w2 + (k & 1) * GSLAB;
#pragma unroll
        for (int i = 0; i < GWPT; i++) s_w[tid + i * GNT] = rw[i];
        fetch_slab(k + 1 < NCH ? k + 1 : 0);
        __syncthreads();
        return s_w;
    };
    // accumulators start AT the bias (read again for every pass: cache hits, and eight registers less across the pass): tile nt
    // of the pair packing holds channels (nt >> 1) * 32 + 8 g + (nt & 1) * 4 + [0, 4)
    auto bias_of = [&](const float *b, int nt) { return *reinterpret_cast<const f32x4 *>(b + (nt >> 1) * 32 + g * 8 + (nt & 1) * 4); };
    // this lane's 16-byte slot of a plane row: channels c * 8 + [0, 8) of candidate r (c = 4 u + g), swizzled so that the 16
    // candidates of a lane group, 128 bytes apart, fall on distinct slots of the bank window
    auto slot = [&](int c) { return r * 128 + ((c ^ (r & 7) ^ (r >> 3)) & 7) * 16; };
    uint8_t *mid = s_mid + (size_t)sub * GMID;
    // candidate `slot` of the group's 16 of a pass: (image, pixel); past the list's end its last entry, of which nothing is stored
    auto candidate = [&](int pass, int slot, bool &valid, int &img, int &p) {
        const int k = pass * (GNG * 16) + sub * 16 + slot;
        valid = k < n;
        const int kk = valid ? k : n - 1;
        int lo = 0, hi = batch - 1;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (s_pre[m] > kk) hi = m; else lo = m + 1;
        }
        img = lo;
        const int ent = kk - (img > 0 ? s_pre[img - 1] : 0);
        p = min(max(a.list[(size_t)img * HW + ent], 0), HW - 1);
    };

    // The input fragments are LOADED in another lane mapping than the MFMA reads them in.  The B fragment of lane (g, r) =
    // lane 16 g + r is channels 8 g + [0, 8) of candidate r, so four consecutive lanes would read four pixels: four cache
    // lines, and a load instruction is 64 tag look-ups -- the level's input lines are what a slab step of this kernel waits
    // for, and a pass was bound by them.  Lane l therefore loads channels 8 (l & 3) + [0, 8) of candidate l >> 2 -- four
    // consecutive lanes one 64-byte piece, 16 look-ups per instruction -- and the fragment reaches its MFMA lane by four
    // ds_bpermute_b32 (no LDS memory is touched): lane 16 g + r takes lane 4 r + g's.
    const int from = (r * 4 + g) * 4;
    auto to_mfma_lanes = [&](half8 (&row)[5]) {
#pragma unroll
        for (int j = 0; j < 5; j++) {
            u32x4 v = __builtin_bit_cast(u32x4, row[j]);
#pragma unroll
            for (int d = 0; d < 4; d++) v[d] = (unsigned int)__builtin_amdgcn_ds_bpermute(from, (int)v[d]);
            row[j] = __builtin_bit_cast(half8, v);
        }
    };

    // ---- the keypoint branch: the group's fourth wave, on the group's 16 candidates ----
    // cv4.L.0 at all nine positions (kpt3_kernel's stage 1: the nt = 1 packing straight from memory through a ring of one
    // chunk's nine fragments, refilled filter row by filter row with the next chunk's -- the next pass's first chunk behind the
    // last --, B fragments of the 5 x 5 input pixels straight from memory like the box waves'), cv4.L.1 and the final at the
    // candidate.
    // The wave reads no LDS but its own plane, so it needs none of the barriers; it joins every one of a pass (the chunk slabs',
    // the second conv's two, the final's) to keep the workgroup's count, and places its stages behind them: the second conv
    // reads the plane behind the first slab barrier of the box branch's stage 2, the final reads the activated sums back
    // behind the barrier in front of the box final -- LDS reads, so no MFMA here reads a register that inline asm wrote.
    if constexpr (KPT) {
        if (row == 3) {
            uint8_t *kp = smem + GLDS + (size_t)sub * KMID;
            const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t *>(a.kw0), 0, CH1 * 9 * 1024, 0x00020000);
            auto load_w = [&](int k) { return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, k * 1024, 0)); };   // [chunk][tap][lane]
            half8 A[9];
#pragma unroll
            for (int tap = 0; tap < 9; tap++) A[tap] = load_w(tap);
            const int tap_lo = g >> 1;   // second conv: this lane's tap of k-step ks is 2 ks + tap_lo (the Cin = 16 direct kernel's k-step)
            for (int pass = blockIdx.x; pass * (GNG * 16) < n; pass += gridDim.x) {
                bool valid;
                int img, p;
                candidate(pass, lane >> 2, valid, img, p);   // (the LOAD mapping's candidate, below)
                const int cy = p / W, cx = p - cy * W;
                // the 5 x 5 input pixels: one bit per pixel inside the map (none for a lane past the list's end) and the byte offset
                // of the corner; an offset past the descriptor's range reads zeros.  (25 offsets held in registers spill.)
                unsigned int inside = 0u;
#pragma unroll
                for (int i = 0; i < 5; i++)
#pragma unroll
                    for (int j = 0; j < 5; j++)
                        inside |= (valid && (unsigned)(cy - 2 + i) < (unsigned)H && (unsigned)(cx - 2 + j) < (unsigned)W ? 1u : 0u) << (i * 5 + j);
                const int corner = (((img * H + cy - 2) * W + cx - 2) * a.x_ld + (lane & 3) * 8) * 2;
                // ... all of it for the candidate this lane LOADS for; the MFMA lane (g, r) takes its own candidate's bits and head row
                // (the index: below 2^31 like every offset of the input) from a lane that loaded for candidate r
                const unsigned int inside_m = (unsigned int)__builtin_amdgcn_ds_bpermute(from, (int)inside);
                const int orow = __builtin_amdgcn_ds_bpermute(from, img * HW + p);
                auto src = [&](int i, int j) { return (inside >> (i * 5 + j) & 1u) ? corner + (i * W + j) * a.x_ld * 2 : 0x7fffffff; };
                const f32x4 kb0 = *reinterpret_cast<const f32x4 *>(a.kb0 + g * 4);
                f32x4 acc[9];
#pragma unroll
                for (int q = 0; q < 9; q++) acc[q] = kb0;
                // ---- stage 1: position q = 3 py + px is pixel (cy - 1 + py, cx - 1 + px) ----
                // A chunk is walked by INPUT row: row i feeds the output rows py = i - kh (kh = 0 .. 2) and is dead behind them, so
                // its registers take the next chunk's row i at once -- every request is a whole chunk ahead of its use, only a
                // pass's first chunk waits for its loads, and 25 fragments are all the wave holds.  Rows ascending are filter
                // rows ascending for every output row, so per output element the order is still chunk, then tap.  The weight
                // fragments of filter row kh are free behind input row kh + 2 and take the next chunk's there.  Requests leave
                // in the order their data is needed (the memory counter is in order); the scheduling barriers keep them where
                // they stand (left alone the compiler sinks every load to its first use).
                auto load_row = [&](half8 (&dst)[5], int i, int c) {
#pragma unroll
                    for (int j = 0; j < 5; j++) dst[j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_x, src(i, j), c * 64, 0));
                };
                half8 in[5][5];
#pragma unroll
                for (int i = 0; i < 5; i++) load_row(in[i], i, 0);
                __builtin_amdgcn_sched_barrier(0);
                to_mfma_lanes(in[0]);
                for (int c = 0; c < CH1; c++) {
                    const bool more = c + 1 < CH1;
                    const int cn = more ? c + 1 : 0;
                    __syncthreads();   // (the box waves' stage_slab(c))
#pragma unroll
                    for (int i = 0; i < 5; i++) {
                        // (the row behind this one changes lanes under this row's MFMAs: this chunk's, or the next chunk's row 0)
                        if (i < 4) to_mfma_lanes(in[i + 1]);
                        else if (more) to_mfma_lanes(in[0]);
#pragma unroll
                        for (int py = 0; py < 3; py++) {
                            const int kh = i - py;
                            if (kh < 0 || kh > 2) continue;
#pragma unroll
                            for (int kw = 0; kw < 3; kw++)
#pragma unroll
                                for (int px = 0; px < 3; px++)
                                    acc[py * 3 + px] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[kh * 3 + kw], in[i][px + kw], acc[py * 3 + px], 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (more) load_row(in[i], i, c + 1);
                        if (i >= 2) {
#pragma unroll
                            for (int kw = 0; kw < 3; kw++) A[(i - 2) * 3 + kw] = load_w(cn * 9 + (i - 2) * 3 + kw);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
                for (int q = 0; q < 9; q++) {
                    const int py = q / 3, px = q - py * 3;
                    half4 o = silu_pack4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
                    if (!(inside_m >> ((py + 1) * 5 + px + 1) & 1u)) o = (half4){0, 0, 0, 0};   // outside the map: the second conv's zero padding (a lane past the list's end: all zero)
                    *reinterpret_cast<half4 *>(kp + q * KROW + r * 32 + g * 8) = o;
                }
                __syncthreads();   // (stage_slab(CH1))
                // ---- stage 2: five k-steps of two taps, the tenth tap zero in A and B ----
                {
                    const half8 *w2p = reinterpret_cast<const half8 *>(a.kw1);   // Cin = 16 direct packing: [k-step][lane], 288 fragments
                    f32x4 c1 = *reinterpret_cast<const f32x4 *>(a.kb1 + g * 4);
                    half8 A2[5], B2[5];
#pragma unroll
                    for (int ks = 0; ks < 5; ks++) A2[ks] = w2p[ks * 64 + (ks == 4 ? (lane & 31) : lane)];
                    if (g >= 2) A2[4] = (half8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < 5; ks++) {
                        const int tap = 2 * ks + tap_lo;
                        const half8 q = *reinterpret_cast<const half8 *>(kp + (tap < 9 ? tap : 0) * KROW + r * 32 + (g & 1) * 16);
                        B2[ks] = tap < 9 ? q : (half8){0, 0, 0, 0, 0, 0, 0, 0};
                    }
#pragma unroll
                    for (int ks = 0; ks < 5; ks++) c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(A2[ks], B2[ks], c1, 0, 0, 0);
                    *reinterpret_cast<half4 *>(kp + 9 * KROW + r * 32 + g * 8) = silu_pack4(c1[0], c1[1], c1[2], c1[3]);
                }
                // ---- the final 1x1: the Cin = 16 direct kernel's K16_FUSE epilogue (its weights and bias requested in front of the barriers) ----
                {
                    const half4 w3f = *reinterpret_cast<const half4 *>(a.kw2 + lane * 4);
                    int g4 = g * 4;
                    asm volatile("" : "+v"(g4));   // (not loop-invariant to the compiler: it would keep the lane's two 64-bit addresses below across the pass, in scratch)
                    const f32x4 b3 = *reinterpret_cast<const f32x4 *>(a.kb2 + g4);
                    __syncthreads();   // (stage_slab(CH1 + 1))
                    __syncthreads();   // (the barrier in front of the box final)
                    const half4 B = *reinterpret_cast<const half4 *>(kp + 9 * KROW + r * 32 + g * 8);
                    const f32x4 c2 = __builtin_amdgcn_mfma_f32_16x16x16f16(w3f, B, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    const f32x4 v2 = (f32x4){c2[0] * kActUnscale + b3[0], c2[1] * kActUnscale + b3[1], c2[2] * kActUnscale + b3[2], c2[3] * kActUnscale + b3[3]};
                    if (inside_m >> 12 & 1u) *reinterpret_cast<f32x4 *>(a.kout + (size_t)orow * a.kout_ld + g4) = v2;   // (the candidate itself is inside the map: the bit is `valid`)
                }
            }
            return;
        }
    }
    fetch_slab(0);

    for (int pass = blockIdx.x; pass * (GNG * 16) < n; pass += gridDim.x) {
        bool valid;
        int img, p;
        candidate(pass, lane >> 2, valid, img, p);   // (the candidate this lane LOADS for: the load mapping, above)
        const int cy = p / W, cx = p - cy * W;

        f32x4 acc[3][4];
        int src[3][5];        // byte offsets of the wave's 3 x 5 input pixels (kpt3_kernel's descriptor loads: an offset past the range reads zeros)
#pragma unroll
        for (int kh = 0; kh < 3; kh++)
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const int iy = cy + row - 2 + kh, ix = cx - 2 + j;
                const bool in = valid && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                src[kh][j] = in ? (((img * H + iy) * W + ix) * a.x_ld + (lane & 3) * 8) * 2 : 0x7fffffff;
            }
        // the MFMA lane (g, r) takes what it needs of ITS candidate r from a lane that loaded for it: the three positions inside
        // the map, `valid`, and the head row
        int mine = valid ? 8 : 0;
#pragma unroll
        for (int i = 0; i < 3; i++) mine |= ((unsigned)(cy + row - 1) < (unsigned)H && (unsigned)(cx + i - 1) < (unsigned)W ? 1 : 0) << i;
        mine = __builtin_amdgcn_ds_bpermute(from, mine);
        const int head_row = __builtin_amdgcn_ds_bpermute(from, img * HW + p);   // (below 2^31 like every offset of the input)
        valid = (mine & 8) != 0;
        bool inmap[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            inmap[i] = (mine >> i & 1) != 0;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) acc[i][nt] = bias_of(a.b0, nt);
        }

        // ---- stage 1: the first 3x3 at the nine positions, chunk by chunk ----
#pragma unroll 1   // (unrolled -- the compiler's choice at Cin = 64 and 128 -- the stage-1 waves spill)
        for (int c = 0; c < CH1; c++) {
            half8 in[3][5];
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
                for (int j = 0; j < 5; j++) in[kh][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_x, src[kh][j], c * 64, 0));
            const half8 *s_w = stage_slab(c);
#pragma unroll
            for (int kh = 0; kh < 3; kh++) to_mfma_lanes(in[kh]);
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int kh = tap / 3, kw = tap - kh * 3;
                half8 A[4];
#pragma unroll
                for (int nt = 0; nt < 4; nt++) A[nt] = s_w[(tap * 4 + nt) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int nt = 0; nt < 4; nt++) acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[nt], in[kh][i + kw], acc[i][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                half8 o = silu_pack8(acc[i][2 * u][0], acc[i][2 * u][1], acc[i][2 * u][2], acc[i][2 * u][3],
                                     acc[i][2 * u + 1][0], acc[i][2 * u + 1][1], acc[i][2 * u + 1][2], acc[i][2 * u + 1][3]);
                if (!inmap[i]) o = (half8){0, 0, 0, 0, 0, 0, 0, 0};   // outside the map: the second conv's zero padding
                *reinterpret_cast<half8 *>(mid + (row * 3 + i) * GROW + slot(u * 4 + g)) = o;
            }

        // ---- stage 2: the second 3x3 at the candidates (the group's first wave) ----
        f32x4 acc2[4] = {bias_of(a.b1, 0), bias_of(a.b1, 1), bias_of(a.b1, 2), bias_of(a.b1, 3)};
        for (int u = 0; u < 2; u++) {
            const half8 *s_w = stage_slab(CH1 + u);
            if (row == 0) {
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    half8 A[4];
#pragma unroll
                    for (int nt = 0; nt < 4; nt++) A[nt] = s_w[(tap * 4 + nt) * 64 + lane];
                    const half8 B = *reinterpret_cast<const half8 *>(mid + tap * GROW + slot(u * 4 + g));
#pragma unroll
                    for (int nt = 0; nt < 4; nt++) acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[nt], B, acc2[nt], 0, 0, 0);
                }
            }
        }
        if (row == 0) {   // (the wave's own reads of the plane are behind it: its first rows take the activated sums)
#pragma unroll
            for (int u = 0; u < 2; u++)
                *reinterpret_cast<half8 *>(mid + slot(u * 4 + g)) = silu_pack8(acc2[2 * u][0], acc2[2 * u][1], acc2[2 * u][2], acc2[2 * u][3],
                                                                               acc2[2 * u + 1][0], acc2[2 * u + 1][1], acc2[2 * u + 1][2], acc2[2 * u + 1][3]);
        }
        __syncthreads();

        // ---- the final 1x1 (the group's second wave): lane (g, r) reads channels 32 u + 8 g + [0, 8) of candidate r, the B
        // fragment of k-step u -- the operands and the arithmetic of conv3x3_lds_body's N2 = 4 epilogue ----
        if (row == 1) {
            const half8 *w2 = reinterpret_cast<const half8 *>(a.w2) + lane;
            const half8 B0 = *reinterpret_cast<const half8 *>(mid + slot(g)), B1 = *reinterpret_cast<const half8 *>(mid + slot(4 + g));
            float *orow = a.out + (size_t)head_row * a.out_ld;
#pragma unroll
            for (int t2 = 0; t2 < 4; t2++) {
                f32x4 c2 = (f32x4){0.f, 0.f, 0.f, 0.f};
                c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[(t2 * 2 + 0) * 64], B0, c2, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[(t2 * 2 + 1) * 64], B1, c2, 0, 0, 0);
                const int co = t2 * 16 + g * 4;
                const f32x4 b2 = *reinterpret_cast<const f32x4 *>(a.b2 + co);
                const f32x4 v2 = (f32x4){c2[0] * kActUnscale + b2[0], c2[1] * kActUnscale + b2[1], c2[2] * kActUnscale + b2[2], c2[3] * kActUnscale + b2[3]};
                if (valid) *reinterpret_cast<f32x4 *>(orow + co) = v2;
            }
        }
    }
}

bool box_gather_eligible(int cin) { return cin == 64 || cin == 128 || cin == 256; }

template <int KC>
static void launch_box_gather_inst(const BoxGatherArgs &a, int batch, int grid, hipStream_t s)
{
    if (a.kw0 != nullptr) launch_lds<box_gather_kernel<KC, true>>(dim3(grid), dim3(GNTK), GLDSK, GLDSK, s, a, batch);   // the keypoint branch rides along: a fourth wave per group and its planes
    else launch_lds<box_gather_kernel<KC, false>>(dim3(grid), dim3(GNT), GLDS, GLDS, s, a, batch);
}

bool launch_box_gather(const BoxGatherArgs &a, int cin, int batch, int grid, hipStream_t s)
{
    if (batch < 1 || batch > GMAXB || grid < 1) return false;
    switch (cin) {
    case 64: launch_box_gather_inst<1>(a, batch, grid, s); return true;
    case 128: launch_box_gather_inst<2>(a, batch, grid, s); return true;
    case 256: launch_box_gather_inst<4>(a, batch, grid, s); return true;
    default: return false;
    }
}

}  // namespace irmv
