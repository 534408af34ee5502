// The box branch of one Detect level -- 3x3 (Cin -> 64), 3x3 (64 -> 64), 1x1 (64 -> 64) -- at the step's CANDIDATE ANCHORS only.
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
//             fragments (the rows of a 5 x 5 neighbourhood are L2 hits between the waves); SiLU, fp16, into an LDS plane
//             [position][candidate][64 channels] -- ZERO where the position lies outside the map (the second conv's padding)
//   stage 2   cv2.L.1 at the candidates out of that plane (the group's first wave), SiLU, fp16, into the plane's first rows
//   final     the 1x1 (the group's second wave, behind a barrier: its B fragments are LDS reads, so no MFMA of this file
//             reads a register that inline asm wrote and no mfma_operand_fence is needed), * ln 2 + bias, four f32x4 stores
//             per lane into the head row's box channels
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

#include <mutex>

namespace irmv {

namespace {
constexpr int GNG = 2;                    // candidate groups per pass
constexpr int GNT = GNG * 192;            // three waves per group
constexpr int GSLAB = 9 * 4 * 64;         // half8 of a chunk slab: [tap][tile][lane], 36 KiB
constexpr int GWPT = GSLAB / GNT;         // ... per thread
constexpr int GROW = 16 * 128;            // bytes of a position of the plane: [candidate][64 channels]
constexpr int GMID = 9 * GROW;            // bytes of a group's plane
constexpr int GMAXB = 1024;               // images of a launch (the prefix lives in LDS)
constexpr size_t GWLDS = (size_t)2 * GSLAB * 16;   // two chunk slabs of weights: the MFMAs run on one while the next is written
constexpr size_t GLDS = GWLDS + (size_t)GNG * GMID + (size_t)GMAXB * 4;
static_assert(GSLAB % GNT == 0, "every thread stages the same number of slab pieces");
static_assert(GLDS <= 160 * 1024, "a CU's LDS");   // (ONE workgroup per CU, by the register file too: 254 VGPRs; bounded to 168 the stage-1 waves spill)
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

// STEPS = Cin / 64 (1, 2, 4)
template <int STEPS>
__global__ __launch_bounds__(GNT) void box_gather_kernel(BoxGatherArgs a, int batch)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    half8 *s_w2 = reinterpret_cast<half8 *>(smem);                // two chunk slabs of weights: slab k of a pass in buffer k & 1 (a pass has an even number)
    uint8_t *s_mid = smem + GWLDS;                                // the groups' planes
    int *s_pre = reinterpret_cast<int *>(smem + GWLDS + (size_t)GNG * GMID);   // inclusive prefix of the images' counts
    constexpr int CH1 = 2 * STEPS, NCH = CH1 + 2;                 // chunk slabs of a pass: the first conv's, then the second conv's two
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = wave / 3, row = wave - sub * 3;
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
    fetch_slab(0);

    for (int pass = blockIdx.x; pass * (GNG * 16) < n; pass += gridDim.x) {
        // ---- this lane's candidate ----
        const int k = pass * (GNG * 16) + sub * 16 + r;
        const bool valid = k < n;
        const int kk = valid ? k : n - 1;
        int lo = 0, hi = batch - 1;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (s_pre[m] > kk) hi = m; else lo = m + 1;
        }
        const int img = lo;
        const int ent = kk - (img > 0 ? s_pre[img - 1] : 0);
        const int p = min(max(a.list[(size_t)img * HW + ent], 0), HW - 1);
        const int cy = p / W, cx = p - cy * W;

        f32x4 acc[3][4];
        int src[3][5];        // byte offsets of the wave's 3 x 5 input pixels (kpt3_kernel's descriptor loads: an offset past the range reads zeros)
        bool inmap[3];
#pragma unroll
        for (int kh = 0; kh < 3; kh++)
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const int iy = cy + row - 2 + kh, ix = cx - 2 + j;
                const bool in = valid && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                src[kh][j] = in ? (((img * H + iy) * W + ix) * a.x_ld + g * 8) * 2 : 0x7fffffff;
            }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            inmap[i] = (unsigned)(cy + row - 1) < (unsigned)H && (unsigned)(cx + i - 1) < (unsigned)W;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) acc[i][nt] = bias_of(a.b0, nt);
        }

        // ---- stage 1: the first 3x3 at the nine positions, chunk by chunk ----
        for (int c = 0; c < CH1; c++) {
            half8 in[3][5];
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
                for (int j = 0; j < 5; j++) in[kh][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_x, src[kh][j], c * 64, 0));
            const half8 *s_w = stage_slab(c);
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
            float *orow = a.out + ((size_t)img * HW + p) * a.out_ld;
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

bool launch_box_gather(const BoxGatherArgs &a, int cin, int batch, int grid, hipStream_t s)
{
    if (batch < 1 || batch > GMAXB || grid < 1) return false;
    static std::mutex mu;
    static unsigned long long done[3] = {0, 0, 0};   // per instantiation: the devices whose dynamic-LDS limit has been raised
    auto go = [&](auto kernel, unsigned long long &mask) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!(mask >> (dev & 63) & 1ull)) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GLDS);
                mask |= 1ull << (dev & 63);
            }
        }
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(GNT), GLDS, s, a, batch);
    };
    switch (cin) {
    case 64: go(box_gather_kernel<1>, done[0]); return true;
    case 128: go(box_gather_kernel<2>, done[1]); return true;
    case 256: go(box_gather_kernel<4>, done[2]); return true;
    default: return false;
    }
}

}  // namespace irmv
