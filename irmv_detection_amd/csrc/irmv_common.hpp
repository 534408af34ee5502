// Shared declarations of the gfx950 kernels and their host launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace irmv {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// 16 bytes as the memory instructions move them: eight fp16 of a fragment, loaded, selected and stored without a type
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ld16(const half_t *p) { return *reinterpret_cast<const u32x4 *>(p); }
__device__ __forceinline__ u32x4 keep_if(bool c, u32x4 v) { return c ? v : (u32x4){0u, 0u, 0u, 0u}; }   // zero padding by select (the load itself is unconditional)
__device__ __forceinline__ half8 as_h8(u32x4 v) { return __builtin_bit_cast(half8, v); }

// ---- dynamic LDS above the default 64 KiB (host) ------------------------------------------------------------------------
// A kernel may only be launched with more once hipFuncSetAttribute has raised its limit, per device.  Engines are created
// and run from several threads (one per GPU): the check, the attribute call and the update are one critical section, so no
// thread launches before the limit is raised.  (Taken on every launch CALL -- engine creation, tuning, graph capture, eager
// profiling; a captured step is replayed without any of this code.)
inline std::mutex g_lds_limit_mu;
// The memory of one kernel, per device: the largest byte count granted, and the one value its launcher derives from the
// raised limit (0 where it derives none)
struct LdsGrant { size_t bytes; int derived; };
template <auto Kernel>
inline LdsGrant g_lds_grant[64] = {};
// The limit of `Kernel` on the current device is at least `bytes` afterwards; false: the runtime refused (no sticky error is
// left).  A request at or below the largest count granted does nothing.  derive(dev) runs behind every attribute call,
// inside the critical section (so once per device, unless the runtime refuses); every call hands its value back in `derived`.
template <auto Kernel, class F>
bool raise_lds_limit(size_t bytes, int &derived, F derive)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    LdsGrant &g = g_lds_grant<Kernel>[dev & 63];
    bool ok = true;
    std::lock_guard<std::mutex> lk(g_lds_limit_mu);
    if (bytes > g.bytes) {
        ok = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
        if (ok) g.bytes = bytes;
        else (void)hipGetLastError();
        g.derived = derive(dev);
    }
    derived = g.derived;
    return ok;
}
template <auto Kernel>
bool raise_lds_limit(size_t bytes)
{
    int none;
    return raise_lds_limit<Kernel>(bytes, none, [](int) { return 0; });
}
// ... and the launch behind it (a refusal shows as the launch's own error)
template <auto Kernel, class... A>
void launch_lds(dim3 grid, dim3 block, size_t lds, size_t limit, hipStream_t s, A... args)
{
    (void)raise_lds_limit<Kernel>(limit);
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
}

// ---- activation scale (round 4) ---------------------------------------------------
// Every fp16 activation tensor between the layers holds a' = log2(e) * a.  With biases pre-multiplied by log2(e) at load
// time (weights unchanged) a SiLU layer's accumulator is y = log2(e) * x, and
//     log2(e) * x * sigmoid(x) = y * rcp(1 + exp2(-y)):
// v_exp_f32 (with a free negate modifier), v_add, v_rcp, v_pk_mul, v_cvt_pk -- the v_mul in front of the exponential that
// exp(-x) = exp2(-x * log2 e) costs per output value is gone, and so is the bias add (accumulators start AT the bias).
// model.0 reads the unscaled image: its epilogue scales the accumulator (one fma, the bias rides in it); the Detect
// finals (no activation, fp32 out) undo the scale the same way: out = acc * ln 2 + bias.  Read-backs of activation
// tensors multiply by ln 2 on the host (engine.cpp read_tensor_f32).
// RANGE: a stored activation overflows fp16 where log2(e) * |a| > 65504, i.e. at |a| > 45 403 instead of 65 504 (it becomes
// +-inf, as a plain fp16 pipeline's does above 65 504; nothing saturates).  Trained detection networks keep activations
// within a few hundred; tests/test_gpu_engine.py::test_activation_range_under_the_log2e_scale pins the behaviour on both sides
// of the edge (finite and equal to the fp16-emulating oracle's at 4e4, inf past 45.4e3).  sppf_pool's v_pk_max_f16 assumes
// no NaN: an inf is ordered like any value, a NaN (inf - inf in a later layer) can only arise past that edge.
constexpr float kActScale = 1.44269504088896341f;    // log2(e)
constexpr float kActUnscale = 0.693147180559945309f; // ln 2
// Rounding is pinned by hand.  Left to the compiler, (half)(y * r) becomes v_pk_mul_f32 + v_cvt_pk_f16_f32 (two roundings)
// where a lane's values pair up in registers and v_fma_mixlo/hi_f16 (the exact product rounded ONCE) where one is left
// over -- which values those are differs from kernel to kernel, so two kernels computing the same layer disagreed in one
// output of 70 000.  Every SiLU output is therefore produced by v_fma_mix*_f16 explicitly: exp, add, rcp, fma_mix -- four
// vector instructions per output value, no separate multiply or convert -- and the shortcut variants (activation + residual,
// rounded after the add) pin their fp32 intermediates with empty asm statements.
__device__ __forceinline__ float silu_rcp(float y) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-y)); }
// two activated outputs as one packed half2: lo = half(y0 * sigma(y0)), hi = half(y1 * sigma(y1)), each rounded once
__device__ __forceinline__ unsigned int silu_pack2(float y0, float y1)
{
    const float r0 = silu_rcp(y0), r1 = silu_rcp(y1);
    unsigned int o;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(o) : "v"(y0), "v"(r0));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(o) : "v"(y1), "v"(r1));
    return o;
}
__device__ __forceinline__ half8 silu_pack8(float y0, float y1, float y2, float y3, float y4, float y5, float y6, float y7)
{
    return as_h8((u32x4){silu_pack2(y0, y1), silu_pack2(y2, y3), silu_pack2(y4, y5), silu_pack2(y6, y7)});
}
__device__ __forceinline__ half4 silu_pack4(float y0, float y1, float y2, float y3)
{
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(half4, (u32x2_t){silu_pack2(y0, y1), silu_pack2(y2, y3)});
}
// An MFMA that takes a SiLU output as its A / B operand straight from the registers (the fused finals of k_conv.hip): the
// hardware needs two wait states between a vector-ALU write of a VGPR and an MFMA's read of it, and the compiler, which
// inserts them for instructions it knows, does not look inside the inline asm above -- with the last v_fma_mixhi_f16 one
// instruction in front of the MFMA the matrix pipe read the register's OLD value (round 5: the keypoint final came out
// wrong in 60 % of its outputs).  These ties put an `s_nop 1` between the asm's writes and whatever reads the value next.
__device__ __forceinline__ void mfma_operand_fence(half4 &x) { asm volatile("s_nop 1" : "+v"(x)); }
__device__ __forceinline__ void mfma_operand_fence(half8 &x, half8 &y) { asm volatile("s_nop 1" : "+v"(x), "+v"(y)); }
// shortcut layers: half(round32(y * sigma(y)) + res), every intermediate rounded where it is written
__device__ __forceinline__ half_t silu_add_res(float y, float res)
{
    float p = y * silu_rcp(y);
    asm("" : "+v"(p));
    float s = p + res;
    asm("" : "+v"(s));
    return (half_t)s;
}

// Workgroup id -> (tile, image) with all tiles of an image on ONE XCD.  The hardware deals consecutive workgroup ids to the 8
// XCDs in turn, and each XCD has its own L2: with the plain (tile, image) grid every neighbour of a tile runs on another XCD
// and re-reads the shared halo from memory (profiles/r04_traffic.json: 1.25 - 1.45 x the algorithmic bytes in the fused C2f kernels, 1.30 x in the front kernel).
// Here id = 8 j + x  ->  image 8 (j / tiles) + x, tile j % tiles: XCD x walks whole images, their halos meet in its L2.
// The batch's last (batch % 8) images take the plain order.  `xcd` = 0 switches the mapping off (IRMV_XCD_IMAGES=0).
__device__ __forceinline__ void tile_image(int id, int tiles, int batch, int xcd, int &tile, int &image)
{
    const int full = xcd ? (batch >> 3) * 8 * tiles : 0;
    if (id < full) {
        const int j = id >> 3;
        image = (j / tiles) * 8 + (id & 7);
        tile = j % tiles;
    } else {
        const int r = id - full;
        image = (full / tiles) + r / tiles;
        tile = r % tiles;
    }
}

// host side: the mapping is on unless IRMV_XCD_IMAGES=0 (read at every launch CALL: engine creation, tuning, graph capture)
inline int xcd_image_order()
{
    const char *v = getenv("IRMV_XCD_IMAGES");
    return (v && v[0] == '0') ? 0 : 1;
}

// lockstep resident-weight 3x3 kernel: waves 4 .. 7 defer their epilogue by one image (k_conv.hip); IRMV_WRES_STAGGER=0: off
inline int wres_stagger()
{
    const char *v = getenv("IRMV_WRES_STAGGER");
    return (v && v[0] == '0') ? 0 : 1;
}

constexpr int kHeadRec = 96;   // fp32 per anchor: box 64 | cls 16 (nc<=16) | kpt 16 (nk<=16)
constexpr int kClsOff = 64;
constexpr int kKptOff = 80;
constexpr int kCandCap = 8192; // == IRMV_CAND_CAP
constexpr int kMaxDetCap = 256;

// ---- preprocess ------------------------------------------------------------
// One bilinear tap table entry per destination coordinate (built on the host
// with the integer arithmetic of the oracle's axis_tap; rotate180 already folded
// into i0/i1).  i0 < 0 marks a letterbox pad coordinate.
struct AxisTap { int32_t i0, i1, w1, pad; };

struct PreArgs {
    const uint8_t *src;   // [B][sh][sw][3]
    half_t *dst;          // [B][net_h][net_w][4]
    const AxisTap *tx, *ty;   // [net_w], [net_h]
    int sw, sh, net_w, net_h, swap_rb;
    size_t src_slot_bytes;
};
void launch_preprocess(const PreArgs &a, int batch, hipStream_t s);
void launch_rotate180(const uint8_t *src, uint8_t *dst, int sw, int sh, hipStream_t s);
void launch_upload_frames(const uint8_t *src_host_mapped, uint8_t *dst, size_t bytes, int blocks, hipStream_t s);   // bytes % 16 == 0, both pointers 16-byte aligned

// ---- raw Bayer input (k_bayer.hip) ---------------------------------------------------
// uint8 [B][H][W] CFA frames -> HWC [B][H][W][3] (R, G, B): integer bilinear demosaic with reflect-101 borders, then the
// Q8 white-balance gains (irmv_detection_amd/bayer.py is the bit-exact host reference).  Any alignment of `raw` and `dst`.
// With `table` set the last step per channel is table[c][v] instead (gains and tone LUT folded on the host,
// irmv_engine_set_bayer_isp), and `mhc` selects the 5 x 5 Malvar-He-Cutler interpolation (always in the table form).
constexpr int kBayerBandRows = 8;   // output rows per workgroup (+ one halo row above and below, two for MHC, staged in LDS)
constexpr int kBayerTableBytes = 3 * 256;
struct BayerArgs {
    const uint8_t *raw;       // [B][H][W]
    uint8_t *dst;             // [B][H][W][3]
    size_t raw_slot_bytes, dst_slot_bytes;
    int W, H;                 // both even
    int ry, rx;               // row / column parity of the R sites (B at the opposite parities)
    uint32_t gain[3];         // Q8, 256 = identity
};
void launch_demosaic(const BayerArgs &a, int batch, hipStream_t s);
void launch_demosaic_table(const BayerArgs &a, const uint8_t *table, bool mhc, int batch, hipStream_t s);   // table: [3][256] device bytes, 16-byte aligned; mhc: W, H >= 4

// tracking window (k_window.hip): frame b's win_w x win_h window at win[first + b] of its full HWC frame -> its compact frame
struct CropArgs {
    const uint8_t *src;       // [num_slots][full_h][full_w][3]: the device frames, or the pinned slots through their device mapping
    uint8_t *dst;             // [num_slots][win_h][win_w][3]
    size_t src_slot_bytes, dst_slot_bytes;
    const int2 *win;          // [num_slots] top-left corner (x, y) in buffer coordinates; read when the kernel runs
    int first;
    int full_w, full_h, win_w, win_h;
    int src_slot;             // -1: frame b is cut out of its own slot's frame; >= 0 (tiled steps): every frame out of this slot's
};
void launch_window_crop(const CropArgs &a, int batch, hipStream_t s);

// model.0.conv: 3x3 s2, 3(+1 pad) -> 16, SiLU
struct Conv0Args {
    const half_t *x;      // [B][net_h][net_w][4]
    half_t *y;            // [B][net_h/2][net_w/2][16]
    const half_t *w;      // packed MFMA A fragments [2 k-steps][64 lanes][8]; k = kh*16 + slot*4 + c
    const float *b;       // [16]
    int net_w, net_h, batch;
};
void launch_conv0(const Conv0Args &a, hipStream_t s);

// fused front: preprocess + model.0.conv + model.1.conv (k_front.hip)
constexpr int kFrontTileY = 4, kFrontTileX = 16;   // model.1 output tile of one workgroup
constexpr int kFrontTileYDirect = 8;               // ... of engines whose tiles all read their source directly (columns at exactly 2 : 1)
constexpr int kFrontStageMax = 128 * 1024;         // most LDS the tile's source region may take (else: the three kernels)
struct FrontArgs {
    const uint8_t *src;   // [B][sh][sw][3]
    size_t src_slot_bytes;
    const AxisTap *tx, *ty;
    int vx0, vx1, vy0, vy1;   // net-input columns / rows with a source tap: [v0, v1) (the rest is letterbox padding)
    int sw, sh, net_w, net_h, swap_rb;
    int fastx, fx_i0, fx_step;   // columns at exactly 2 : 1: column vx0 + k blends the source pair (m, m + 1), m = fx_i0 + fx_step k (fx_step = +-2), weights 1/2; fastx bit 1: tiles without padding read the source straight into registers
    const half_t *w0;     // model.0.conv fragments (Conv0Args::w)
    const float *b0;
    const half_t *w1;     // model.1.conv, direct-family packing (Cin = 16: 5 k-steps x 2 paired tiles)
    const float *b1;
    half_t *out;          // [B][net_h/4][net_w/4][out_ld]
    int out_ld;
    int tiles_x, tiles_y;
    int tile_y;           // kFrontTileY, or kFrontTileYDirect (needs fastx bit 1)
    int stage_bytes;      // dynamic LDS: >= the largest tile's source region (staged path) and >= front_min_stage_bytes(tile_y)
};
int front_min_stage_bytes(int tile_y = kFrontTileY);
bool front_prepare();
bool launch_front(const FrontArgs &a, int batch, hipStream_t s);

// fused model.2 (C2f: cv1, one shortcut Bottleneck of two 3x3 16 -> 16 convs, cv2) (k_c2f.hip)
constexpr int kC2fTile = 16;
struct C2fArgs {
    const half_t *x;      // block input [B][H][W][x_ld], 32 channels used
    int x_ld;
    half_t *out;          // block output [B][H][W][out_ld], 32 channels
    int out_ld;
    int H, W, tiles_x, tiles_y;   // spatial size, tiles per row / column
    const half_t *w_cv1, *w_m1, *w_m2, *w_cv2;   // direct-family packings of the four layers
    const float *b_cv1, *b_m1, *b_m2, *b_cv2;
};
void launch_c2f2(const C2fArgs &a, int batch, hipStream_t s);

// ---- ShuffleNetV2 stage operators (k_shuffle.hip) ------------------------------
struct DwArgs {
    const half_t *x;      // [B][Hin][Win][x_ld], already offset to the first channel
    int x_ld;
    half_t *y;            // [B][Hout][Wout][y_ld], already offset to the first channel
    int y_ld;
    const half_t *w;      // [9][C] fp16, tap-major
    const float *b;       // [C]
    int Hin, Win, Hout, Wout, C, stride;   // C a multiple of 8
};
void launch_dwconv3x3(const DwArgs &a, int batch, hipStream_t s);
struct ShufArgs {
    const half_t *a, *b;  // [pixels][a_ld / b_ld], already offset to the first channel
    int a_ld, b_ld;
    half_t *out;          // [pixels][out_ld]: out[2 i] = a[i], out[2 i + 1] = b[i], i < bc
    int out_ld, bc;       // bc a multiple of 4
    size_t pixels;        // batch * H * W
};
void launch_shuffle_cat(const ShufArgs &a, hipStream_t s);

// ---- implicit-GEMM conv on MFMA ----------------------------------------------
struct ConvSeg {
    const half_t *p;  // base pointer, already offset to the segment's first channel
    int ld;           // channel stride of a pixel, in elements
    int C;            // channels taken from this segment (multiple of 8); 0 = unused
    int shift;        // 1 = the segment is stored at half resolution (nearest 2x upsample folded in)
};

// fused C2f blocks with a 32-channel hidden width (k_c2f.hip): mode 0 = whole block (n = 1), 1 = cv1 + first
// bottleneck, 2 = last bottleneck + cv2 (n = 2)
constexpr int kC2f32TileH = 8, kC2f32TileW = 16;
struct C2f32Args {
    ConvSeg s0, s1;       // block input (modes 0, 1): up to two K segments, s0 optionally at half resolution
    int cin1;             // s0.C + s1.C
    half_t *cat;          // the block's concat buffer [B][H][W][cat_ld]: y0 | y1 | y2 [| y3], 32 channels each
    int cat_ld, prev_coff;   // mode 2: channel offset of the previous bottleneck's output inside cat
    half_t *out;          // block output [B][H][W][out_ld], 64 channels (modes 0, 2)
    int out_ld;
    int H, W, tiles_x, tiles_y;
    const half_t *w_cv1, *w_m1, *w_m2, *w_cv2;   // direct-family packings
    const float *b_cv1, *b_m1, *b_m2, *b_cv2;
};
size_t c2f32_lds_bytes(int mode);
bool launch_c2f32(int mode, bool shortcut, const C2f32Args &a, int batch, hipStream_t s);

// one 64-channel Bottleneck [+ the block's cv2] of a C2f block in one launch, single-frame steps (k_bneck.hip)
constexpr int kBneckTile = 8;
struct BneckArgs {
    const half_t *yin;    // the Bottleneck's input: a 64-channel slice of the block's concat buffer [B][H][W][yin_ld], offset to its first channel
    int yin_ld;
    half_t *ynext;        // mode A: the next 64-channel slice of the concat buffer (same pixel indexing)
    int ynext_ld;
    const half_t *cat;    // mode B: the concat buffer from channel 0 (cv2 reads the slices in front of y_in from here)
    int cat_ld;
    half_t *out;          // mode B: block output [B][H][W][out_ld], 128 channels
    int out_ld;
    int H, W, tiles_x, tiles_y;
    const half_t *w_m1, *w_m2;   // LDS-family nt = 1 packing [4 tiles][2 chunks][9 taps][64 lanes][8]
    const float *b_m1, *b_m2;
    const half_t *w_cv2;         // direct-family packing [8 tiles][k-steps][64 lanes][8]
    const float *b_cv2;
};
size_t bneck64_lds_bytes(int mode, int ks2);
bool launch_bneck64(int mode, int ks2, bool shortcut, const BneckArgs &a, int batch, hipStream_t s);   // mode 0: A (-> concat slice), 1: B (+ cv2, ks2 = 6 / 8)

// the keypoint branch of one Detect level (3x3 Cin -> 16, 3x3 16 -> 16, 1x1 16 -> nk) in one launch (k_kpt.hip)
constexpr int kKpt3Tile = 10;
struct Kpt3Args {
    const half_t *x;      // the level's input [B][H][W][x_ld], offset to the first of its Cin channels
    int x_ld;
    int H, W, tiles_x, tiles_y;
    const half_t *w1;     // first conv: LDS-family nt = 1 packing [chunk of 32][tap][64 lanes][8]
    const float *b1;
    const half_t *w2;     // second conv: Cin = 16 direct packing [5 k-steps][64 lanes][8]
    const float *b2;
    const half_t *w3;     // final 1x1: A layout of v_mfma_f32_16x16x16_f16 [64 lanes][4]
    const float *b3;      // (not scaled: the final has no activation)
    float *out;           // head records [B][H * W][out_ld], offset to the keypoint channels
    int out_ld;
    const unsigned int *cand_bits;   // sparse head: [B][cand_words] candidate-anchor bitmap, rows of other anchors are not stored; nullptr = all rows
    int cand_words, abase;           // abase: first anchor index of this level
    int tile_gate;                   // sparse branch (with cand_bits): != 0 = a (tile, image) pair without a candidate anchor in the tile is not computed
};
bool kpt3_eligible(int cin);
bool launch_kpt3(const Kpt3Args &a, int cin, int batch, hipStream_t s);

// The box branch of one Detect level (3x3 Cin -> 64, 3x3 64 -> 64, 1x1 64 -> 64) at the step's candidate anchors only, from a
// compact list (k_boxg.hip).  cand_list_kernel writes the lists of all levels: per image of the launch its candidate pixels
// of the level, in any order, and their number.
struct CandListArgs {
    const unsigned int *cand_bits;   // [B][cand_words] candidate-anchor bitmap
    int cand_words;
    int abase[3], hw[3];             // first anchor and pixel count of each level
    int *list[3];                    // [B][hw] pixel y * W + x; nullptr: the level keeps no list
    int *count[3];                   // [B]
};
void launch_cand_list(const CandListArgs &a, int batch, hipStream_t s);
struct BoxGatherArgs {
    const half_t *x;      // the level's input [B][H][W][x_ld], offset to the first of its Cin channels
    int x_ld;
    int H, W;
    const half_t *w0;     // first conv: LDS-family nt = 4 packing [chunk of 32][tap][4 tiles][64 lanes][8]
    const float *b0;
    const half_t *w1;     // second conv: the same packing, two chunks
    const float *b1;
    const half_t *w2;     // final 1x1: [4 tiles][2 k-steps][64 lanes][8]
    const float *b2;      // (not scaled: the final has no activation)
    float *out;           // head records [B][H * W][out_ld], offset to the box channels
    int out_ld;
    const int *list;      // [B][H * W], const int *count: [B] (CandListArgs)
    const int *count;
    // the level's keypoint branch in the same launch (Kpt3Args' operands w1 .. b3 and out); kw0 == nullptr: box only
    const half_t *kw0;    // first conv: LDS-family nt = 1 packing [chunk of 32][tap][64 lanes][8]
    const float *kb0;
    const half_t *kw1;    // second conv: Cin = 16 direct packing [5 k-steps][64 lanes][8]
    const float *kb1;
    const half_t *kw2;    // final 1x1: A layout of v_mfma_f32_16x16x16_f16 [64 lanes][4]
    const float *kb2;
    float *kout;          // head records, offset to the keypoint channels
    int kout_ld;
};
bool box_gather_eligible(int cin);
bool launch_box_gather(const BoxGatherArgs &a, int cin, int batch, int grid, hipStream_t s);   // grid: the persistent workgroups (captured with the step)

// Class policy (irmv_engine_set_class_policy): one logit threshold and one plate model per class, in device memory at an
// address fixed for the engine's life -- kernels hold the pointer, a captured graph never the values.  (anchor, c) is a
// candidate iff logit > thr[c]; min_thr = the smallest thr[c] over c < nc (+inf: every class off), the wave-uniform pre-test
// in front of the per-class compare.  Entries at and above nc are +inf / the configured plate and never read by a compare.
constexpr int kMaxClasses = 16;
struct ClassTable {
    float min_thr;
    int32_t pad_[3];
    float thr[kMaxClasses];
    int32_t plate[kMaxClasses];   // IRMV_ARMOR_*: index into PnpConst::hy / hz for a detection of class c
};

struct ConvArgs {
    ConvSeg s0, s1;
    int Hin, Win;       // input size at the conv's own resolution
    int Hout, Wout;
    int M;              // batch * Hout * Wout
    int Cin;            // s0.C + s1.C
    const half_t *w;    // packed MFMA A fragments [ntile][kstep][64 lanes][8]
    const float *bias;  // [cout_pad]
    void *out;          // half_t* or float*, already offset to the first output channel
    int out_ld;
    const half_t *res;  // optional residual (same pixel indexing as out), nullable
    int res_ld;
    int cout_pad;       // multiple of 16
    int ksteps;
    int pair;           // weight rows packed with the paired-tile channel permutation
    // optional trailing 1x1 conv fused into the epilogue of the LDS 3x3 kernel (Detect-head finals: bias only, fp32
    // out): this conv's activated fp16 output never leaves the registers.  n2 = 16-row tiles of the 1x1 (0 = none).
    // (Cin = 16 direct kernel, keypoint branch: w2 = the 16 -> nk final in the 16x16x16 MFMA's A layout [64 lanes][4], n2 = 1.)
    const half_t *w2;   // direct-family packing of the 1x1 [tile][k-step][64][8], Cin = this conv's 64 channels
    const float *bias2;
    float *out2;
    int out2_ld, n2;
    // Detect class branch only (the fused 1x1 IS the class-logit conv): candidates are thresholded where the logits are
    // computed and appended to the frame's key list -- the separate scan over the head tensor then never runs.
    unsigned long long *scan_keys;   // [B][scan_key_cap], nullptr = off
    int *scan_counts;                // [B]
    const ClassTable *scan_cls;      // per-class thresholds (never null where scan_keys is set)
    int scan_nc, scan_abase, scan_key_cap;   // classes; first anchor index of this level; list capacity (= A * nc)
    // Sparse head (LDS 3x3 kernel, N2 > 0): the frame's candidate-anchor bitmap, one bit per anchor.  nullptr = every head row
    // is stored.  With scan_keys (class carrier): a candidate's anchor bit is set next to its key and the class channels are
    // not stored at all (the score travels in the key).  Without (box carrier, launched behind its level's class carrier):
    // a row is stored only where the anchor's bit is set; scan_abase is then the level's anchor base here too.
    unsigned int *cand_bits;         // [B][cand_words]
    int cand_words;
    // Sparse branch (tile gate; the resident-weight 3x3 kernels, every other family ignores it and computes everything): a
    // (tile, image) pair is computed only if some anchor of the level has its bit set inside the tile's output pixels grown by
    // `halo` pixels on every side.  0 = off, 1 = halo 0 (box carriers: their output is head rows), 2 = halo 1 (the box branch's
    // first conv: the carrier's 3x3 at a candidate pixel reads its 3x3 neighbourhood).  Needs cand_bits, cand_words and
    // scan_abase (the level's anchor base), also on a conv without a fused 1x1; the launch must stand behind the level's class
    // carrier.  What is stored never depends on it: rows are gated per anchor as above, a skipped tile only leaves memory as it was.
    int tile_gate;
};

// several independent layers in one launch (k_conv.hip conv3x3_lds_multi / conv_mfma_multi)
constexpr int kMultiMax = 6;
struct LdsMember {
    ConvArgs a;
    const half_t *wl;
    int tiles_x, tiles_y, twc_log2, patch_bytes, batch, tile2d;
    int gx, gy;                 // this member's grid
};
struct LdsMultiArgs {
    int n;
    int start[kMultiMax + 1];   // first workgroup of member k
    LdsMember m[kMultiMax];
};
struct DirectMultiArgs {
    int n;
    int start[kMultiMax + 1], gx[kMultiMax], gy[kMultiMax];
    ConvArgs a[kMultiMax];
};

struct ConvCfg {
    int ks, stride, mt, nt; bool cin16; int act; bool out_f32; bool lds; int ipw;   // ipw: images per workgroup (LDS family)
    bool deep;   // direct kernel, latency variant: prefetch ring of 6..12 k-steps (single-frame steps)
    bool ct;     // direct kernel walking K chunk-major with the LDS family's weights: bit-identical stand-in for that family
    bool pw;     // 1x1 layers: the persistent pointwise kernel (weights in LDS, pixel tiles software-pipelined)
    bool pf2;    // LDS family, mt = 1: global -> register staging two (image, chunk) steps ahead instead of one
    bool pf4;    // LDS family, mt = 1, nt = 1: four steps ahead (a lone frame's 128-channel layers: all of a workgroup's steps in flight at once)
    bool w8;     // LDS family, stride 2: one 8-wave workgroup on a block twice as tall (weights staged for twice the pixels, mt = 2 fits LDS)
    int cm;      // LDS family: chunk-major order over the workgroup's cm = ipw images (0: image-major), weights staged once per chunk
    bool wr;     // LDS family, Cin = Cout = 64, stride 1: the layer's weights stay resident in the LDS of one 8-wave workgroup that walks ipw images
    bool pp;     // ... as two ping-pong groups of four waves (one in its MFMA phase while the other stores, stages and loads)
};
// A conv op's weight packings: the direct family's fragments, the LDS family's per-nt packings (nt = 1 / 2 / 4 / 8, nullptr
// where the layer has none: [n-block][chunk 32][tap][tile][lane][8]), and a Cin = 16 final's weights in the A layout of the
// 16x16x16 MFMA (nullptr: not such a final)
struct ConvWeights { const half_t *w_packed; const half_t *w_lds[4]; const half_t *w_k16; };
// The one answer to "which kernel runs cfg on this layer" (k_conv.hip's variant tables): false = no such variant.  Launches
// nothing; out (optional) receives the launcher, its weights, geometry and dynamic LDS (unspecified on false).
struct ConvLaunch;
bool resolve_conv(const ConvCfg &cfg, const ConvArgs &a, const ConvWeights &w, int batch, ConvLaunch *out = nullptr);
bool launch_conv(const ConvCfg &cfg, const ConvArgs &a, const ConvWeights &w, int batch, hipStream_t s);   // false: no such variant
const char *conv_cfg_name(const ConvCfg &cfg, char *buf, int n);
bool conv_pw_eligible(const ConvCfg &cfg, const ConvArgs &a);   // the 1x1 layers the pointwise family serves
bool conv_lds_fits(const ConvArgs &a, const ConvWeights &w, int stride, int mt, int nt);   // LDS family: packing present, (mt, nt) tile fits
int conv_wres_tiles(const ConvArgs &a, int stride, bool pp);    // weights-resident variant: tile positions per image (0 = not eligible)
// n independent layers (n <= kMultiMax) as ONE launch with a common tile: LDS family, stride 1, mt = 1, nt in {1, 2, 4}
// (fused 1x1s allowed at nt = 4, per member); direct family: the two shapes of the keypoint branch (3x3 Cin = 16 SiLU,
// 1x1 fp32 bias-only; mt = nt = 1).  false: some member has no such tile.
bool launch_conv_lds_multi(int nt, const ConvArgs *a, const ConvWeights *w, int n, int batch, hipStream_t s);
bool launch_conv_direct_multi(const ConvCfg &cfg, const ConvArgs *a, int n, hipStream_t s);

// SPPF pooling chain: slice 0 (C ch) of [B][H][W][4C] -> slices 1..3 (5x5, 9x9, 13x13 max)
void launch_sppf_pool(half_t *buf, int batch, int H, int W, int C, hipStream_t s);
// ... the channel slab of its LDS kernel for that launch (8, 16 or 32), or 0: the global-memory kernel (host only)
int sppf_slab(int batch, int H, int W, int C);

// ---- post-processing -----------------------------------------------------------
struct DevDet {           // device/pinned result record
    float box_net[4];     // xyxy, net-input pixels (EfficientNMS det_boxes)
    float xyxy[4];        // source-frame pixels (parse_output)
    float score;
    int32_t cls, anchor, pnp_ok;
    float kpts_net[8];
    float kpts[8];
    double rvec[3], tvec[3], quat[4];
    int32_t armor_valid;  // 1: kpts hold an armor's four points; 0: none; -1: ROI larger than the label scratch
    int32_t armor_size;   // 0 small / 1 large (classical path: from the light-centre distance)
    int32_t n_lights;     // classical path: lights that passed the gates in this ROI
    int32_t pad_;
};
struct DevFrameOut { int32_t num_dets, n_candidates, overflow, pad; };

struct PnpConst {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    double hy[2], hz[2];   // half extents of the small / large armor (metres)
};

// Pose ambiguity (irmv_engine_set_pose_prior): IPPE's two solutions per armor.  A = the one the min-error rule reports (solution
// 0 unless !(err0 <= err1)), B = the other.  DevAlt is the side record of one detection (the layout of irmv_pose_alt): the
// solution its DevDet does NOT carry.  PosePrior and the per-slot up vectors ([num_slots][3] doubles) live in device memory at
// addresses fixed from the first set_pose_prior on and are read when the kernel runs, like ClassTable and PnpConst.
struct DevAlt {
    double rvec[3], tvec[3], quat[4];
    double err, err_alt;      // rms normalised residual of the reported pose / of this one
    int32_t state;            // 0: pnp_ok == 0, the record is all zero; 1: the DevDet holds A; 2: the prior reported B
    int32_t alt_ok;           // this pose's own finiteness check
};
constexpr int kPoseMinErr = 0, kPosePrior = 1;   // == IRMV_POSE_*
struct PosePrior {
    int32_t mode, pad_;
    double ratio;             // B is eligible iff errB <= ratio * errA
    double s[kMaxClasses];    // per class: the expected n . u (n = column 0 of R: the plate normal pointing away from the camera)
    double s_default;         // ... of a detection without a class (explicit boxes)
};
// What one solve needs of the two tables: the rule's operands as values
struct PoseRule { int mode; double ratio, s, ux, uy, uz; };
__device__ inline PoseRule pose_rule(const PosePrior *p, const double *up, int cls)   // cls < 0: s_default
{
    return PoseRule{p->mode, p->ratio, cls >= 0 ? p->s[cls & (kMaxClasses - 1)] : p->s_default, up[0], up[1], up[2]};
}

struct PostArgs {
    const float *head_all;    // one allocation: [level][slot (all num_slots)][H*W][kHeadRec]
    int slots_total, first;   // level block offset = lvl_base * slots_total records; this step starts at slot `first`
    float *boxes;             // [B][A][4]
    unsigned long long *keys; // [B][key_cap]: every (anchor, class) pair above threshold, unsorted (read back only when a frame
                              // has more candidates than the LDS list holds)
    int key_cap;              // = A * nc: the list can never overflow
    DevDet *dets;             // [B][max_det]
    DevFrameOut *fout;        // [B]
    int net_w, net_h, A, nc, nk;   // net input width x height; A = sum over s in {8, 16, 32} of (net_h / s) (net_w / s)
    const ClassTable *cls;    // per-class logit thresholds and plates (ClassTable; the engine's, or its all-infinite mute twin)
    float iou_thr;
    int max_det, pre_nms_cap;
    // parse_output mapping net -> source frame: x_src = (x - off_x) * scale_x
    float scale_x, scale_y, off_x, off_y;
    const PnpConst *pnp;      // device copy (keeps the kernel-argument struct out of scratch)
    long long *dbg;           // optional [B][8] phase stamps of nms_pnp_kernel (diagnostic builds of the engine only)
    int keys_only;            // 1: the key list comes from the class-branch conv epilogues (ConvArgs::scan_keys): nms_pnp_kernel decodes
                              // the candidates' boxes itself
    int prefilter;            // 1: frames with more than 512 candidates first walk their best 320 .. 512 only (exact: nms_pnp_kernel, "ATTEMPT 0")
    int classwalk;            // 1: frames of up to 512 candidates take nms_pnp_kernel's class-major path (round 4); 0: the round-3 matrix walk (bit-identical)
    int *counts;              // [B] candidates appended by scan_decode_kernel; nullptr: nms_pnp_kernel scans the head itself.
                              // Zero at engine creation; nms_pnp_kernel reads its frame's count and resets it (no memset node, nothing
                              // for another step to find non-zero); every reader clamps it to key_cap
    unsigned int *cand_bits;  // [B][cand_words] candidate-anchor bitmap of the sparse head (ConvArgs::cand_bits), or nullptr: nms_pnp_kernel
    int cand_words;           // clears its frame's words where it resets the count
    int pnp_stride;           // frame b solves with pnp[(first + b) * pnp_stride]: 0 = one record for every slot, 1 = one per slot (window engines)
    // Pose ambiguity: all three null until the first irmv_engine_set_pose_prior (nms_pnp_kernel<false>, today's code and bits);
    // set, nms_pnp_kernel<true> runs: survivor j's other solution goes to alts[b * max_det + j], the prior may pick B
    DevAlt *alts;             // [B][max_det], device or pinned like dets
    const PosePrior *prior;
    const double *up;         // [num_slots][3]: frame b's unit up vector at up[3 * (first + b)]
};
void launch_nms_pnp(const PostArgs &a, int batch, hipStream_t s);
void launch_nms_pnp_alt(const PostArgs &a, int batch, hipStream_t s);   // k_post_alt.hip: a.alts != nullptr (launch_nms_pnp calls it)
constexpr int kScanBlocks = 16;   // workgroups per frame of scan_decode_kernel (more where a 16th of the keys would not fit kScanLdsMax)
constexpr size_t kScanLdsMax = 159 * 1024;   // its dynamic LDS: 160 KiB per workgroup on gfx950, less its static variables
void launch_scan_decode(const PostArgs &a, int batch, hipStream_t s);
void post_limits(int32_t out[16]);   // the candidate counts k_post.hip branches on and the merge kernel's capacities (irmv_post_limits)
// tiled search (k_tiles.hip): the result lists of slots [first, first + count) -- windows of ONE frame -- merged into one
constexpr int kMaxTiles = 16;     // == IRMV_MAX_TILES
struct TileMergeParams { float ios_thr, edge_margin; };   // device memory, read when the kernel runs (irmv_engine_set_tile_merge)
struct TileOut {
    int32_t n_kept, n_in, pad_[2];
    int32_t rec[256][4];          // [kMaxDetCap]: tile, index, cut, 0 of kept record i, in merge order
};
struct TileArgs {
    const DevDet *dets;           // [num_slots][max_det] DEVICE records, window-local; tile t is slot first + t
    const DevFrameOut *fout;      // [num_slots]
    const int2 *win;              // [num_slots] corners in buffer coordinates (CropArgs::win)
    const TileMergeParams *params;
    TileOut *out;
    int first, count, max_det;
    int full_w, full_h, win_w, win_h, rotate180;
};
bool tile_merge_prepare();        // raises the kernel's LDS limit on the current device (outside any capture)
void launch_tile_merge(const TileArgs &a, hipStream_t s);

// ---- classical light extraction (k_light.hip) -------------
constexpr int kLightLdsPoints = 256;         // contours up to this many points are sorted / hulled in LDS
constexpr int kLightLdsImage = 40 * 1024;   // padded label images up to this many bytes live in LDS
constexpr int kLightMaxContours = 1024;   // contours per ROI; more -> armor_valid = -1 (no answer), never a truncated one
constexpr int kLightPointsCap = 4096;     // contour points per detection; more -> no answer as well

// What light_extract_kernel saw in one box, stage by stage (test hook irmv_engine_light_trace; the layout of
// irmv_light_rec / irmv_light_trace in include/irmv_hip.h).  Production launches carry no trace.
struct LightTraceRec {
    float corners[8];                        // minAreaRect corners c[0..7], ROI coordinates, before the sort by y
    float top[2], bottom[2], center[2];      // frame coordinates if ok, else ROI coordinates
    double length;
    int32_t measured, ok, hull_edges, in_lds;   // hull_edges: 0 for the degenerate cases (one or two distinct points, collinear)
};
struct LightTrace {
    int32_t n_contours, n_found, n_points, too_large;   // kept (<= cap); as the scan counted them (cap + 1 = more); points counted past the cap
    int32_t pool_fit, in_lds, rx, ry, rw, rh;
    int32_t max_contours, points_cap, lds_image, lds_points;
    uint64_t label_pool, pool_offset;
    int32_t starts[kLightMaxContours + 1];
    int16_t points[kLightPointsCap][2];      // as trace_border emitted them, contours in discovery order
    int32_t pad_;
    LightTraceRec recs[kLightMaxContours];   // per contour, discovery order; measured = 0: fewer than 5 points (or no answer)
};

// The guided instantiation's two live parameters: device memory, read when the kernel runs (irmv_engine_set_refine)
struct RefineParams { float snap, roi_margin; };

struct LightArgs {
    const uint8_t *frames;   // [B][rows][cols][3] device frames (un-rotated; rotation folded into the fetch)
    size_t frame_bytes;
    int cols, rows, rotate180;
    DevDet *dets;            // [B][max_det]: xyxy in (bbox source when boxes == nullptr), armor fields out
    int max_det;
    const int *num_dets;     // per frame, stride num_dets_stride ints; nullptr -> n_boxes for every frame
    int num_dets_stride, n_boxes;
    const float *boxes;      // optional explicit boxes [n_boxes][4] (irmv_engine_extract_armors)
    signed char *labels;     // [B][label_pool] per-frame pool the padded label images are carved from, in detection order
    size_t label_pool;       // bytes per frame (>= one full-frame ROI)
    short *points;           // [B][max_det][points_cap][2] contour points
    int points_cap;
    short *hulls;            // [B][max_det][points_cap * 2][2] hull scratch
    int binary_threshold;
    float light_min_ratio, light_max_ratio, light_max_angle;
    double min_small_cd, max_small_cd, min_large_cd, max_large_cd;
    const PnpConst *pnp;
    int pnp_armor_size;      // plate of explicit boxes (they have no class) ...
    const ClassTable *cls;   // ... and, boxes == nullptr: the table whose plate[dets[i].cls] a step's detection solves with
    LightTrace *trace;       // [n_boxes] or nullptr (every launch of a step): see LightTrace
    int first, pnp_stride;   // frame b solves with pnp[(first + b) * pnp_stride] (PostArgs::pnp_stride)
    const RefineParams *refine;   // non-null: the guided instantiation (light_extract_kernel<true>): dets[i].kpts are the prior, refined in place
    float *kpts;             // guided: the prior [B][max_det][8].  A step's launch fills it from the records first (refine_prior_kernel);
                             // with explicit boxes the caller has (irmv_engine_refine_points), and the records are output only
    // Pose ambiguity (PostArgs): prior == nullptr launches today's instantiations.  alts may be null with prior set (explicit
    // boxes: the rule runs with s_default, no record leaves)
    DevAlt *alts;            // [B][max_det]
    const PosePrior *prior;
    const double *up;        // [num_slots][3], frame b's at up[3 * (first + b)]
};
void launch_light_extract(const LightArgs &a, int n_boxes_max, int batch, hipStream_t s);
void launch_light_extract_alt(const LightArgs &a, int n_boxes_max, int batch, hipStream_t s);   // k_light_alt.hip: a.prior != nullptr (launch_light_extract calls it)

// ---- debug images (k_render.hip; irmv_engine_render) -----------------------------------------------------------------
// One mark record as the host hands it to the kernel: every coordinate already an integer in OUTPUT pixels (truncated, the
// window's corner subtracted, floor-divided by the scale -- include/irmv_hip.h, "debug images").
constexpr int kRenderBox = 1, kRenderLabel = 2, kRenderArmor = 4;   // RenderMark::flags: what the record draws
struct RenderMark {
    int32_t x1, y1, x2, y2;   // box
    int32_t flags, cls;       // kRender* bits; name / colour index 0..14 (14 = UNKNOWN)
    int32_t px[4], py[4];     // LB, LT, RT, RB
    int32_t pad_[2];
};
// glyph rows and class names, built on the host from the table irmv_render_glyph exposes
struct RenderFont {
    uint8_t glyph[16][8];     // [glyph index][row]
    uint8_t name[16][8];      // [class 0..14][k] -> glyph index
    uint8_t len[16];
};
struct RenderArgs {
    const uint8_t *frame;     // [H][W][3] device frame, un-rotated (rotation folded into the fetch)
    uint8_t *dst;             // [oh][ow][3]
    const RenderMark *marks;  // [n]
    const RenderFont *font;
    int W, H, ow, oh, rotate180, scale, binary, threshold, n;
};
constexpr int kRenderTileW = 64, kRenderTileH = 16;   // output pixels per workgroup (256 threads, 4 pixels of a row each)
void launch_render_view(const RenderArgs &a, hipStream_t s);

// ---- frame metering (k_meter.hip; include/irmv_hip.h, "frame metering") -------------------------------------------------
constexpr int kMeterView = 0, kMeterRaw = 1;   // == IRMV_METER_*
// The options as the kernels read them from device memory when they run (a captured graph holds the address): on = 0 is
// "off" -- the histogram kernel returns at once and the record is all zero.
struct MeterParams { int32_t on, domain, x0, y0, w, h, step, pad_; };
struct MeterStats {           // == irmv_frame_stats
    uint32_t hist[4][256];
    uint32_t n[4];
    int32_t rect[4];
    int32_t domain, step, pad_[2];
};
// Where a rectangle lies.  rect: the clipped (RAW: shrunk) rectangle x, y, w, h in view-local result coordinates; bx, by,
// bw, bh: the same region in the coordinates of the buffer that is read -- the view's HWC frame (pixels), or the raw frame
// (CFA sites; all four even); px, py: VIEW: offset in the region of its first sampled column / row (the sample grid hangs at
// the rectangle's corner in RESULT coordinates, which under rotate180 is the region's far corner); nx, ny: sampled columns
// and rows (RAW: 2 x 2 cells).  Everything 0 where nothing is left.
struct MeterGeom { int32_t rect[4], bx, by, bw, bh, px, py, nx, ny; };
__host__ __device__ inline int meter_step(int step) { return step == 2 || step == 4 ? step : 1; }
// THE geometry: irmv_meter_map returns it, both kernels compute it per frame.  vw x vh: the view's frame; (cx, cy): the
// view's corner inside the raw frame, buffer coordinates (a window slot in the window view; else 0, 0).
__host__ __device__ inline MeterGeom meter_geometry(const MeterParams &p, int vw, int vh, int rot, int cx, int cy)
{
    MeterGeom g{};
    long long x0 = p.x0, y0 = p.y0, x1 = x0 + p.w, y1 = y0 + p.h;
    if (p.w == 0 && p.h == 0) { x0 = 0; y0 = 0; x1 = vw; y1 = vh; }
    x0 = x0 > 0 ? x0 : 0; y0 = y0 > 0 ? y0 : 0;
    x1 = x1 < vw ? x1 : vw; y1 = y1 < vh ? y1 : vh;
    if (x1 <= x0 || y1 <= y0) return g;
    const int st = meter_step(p.step);
    const int rw = (int)(x1 - x0), rh = (int)(y1 - y0);
    const int bx = rot ? vw - (int)x1 : (int)x0, by = rot ? vh - (int)y1 : (int)y0;   // in the view's frame as stored
    if (p.domain != kMeterRaw) {
        g.rect[0] = (int)x0; g.rect[1] = (int)y0; g.rect[2] = rw; g.rect[3] = rh;
        g.bx = bx; g.by = by; g.bw = rw; g.bh = rh;
        g.px = rot ? (rw - 1) % st : 0; g.py = rot ? (rh - 1) % st : 0;
        g.nx = (rw + st - 1) / st; g.ny = (rh + st - 1) / st;
        return g;
    }
    const int ex0 = (bx + cx + 1) & ~1, ex1 = (bx + cx + rw) & ~1, ey0 = (by + cy + 1) & ~1, ey1 = (by + cy + rh) & ~1;
    if (ex1 <= ex0 || ey1 <= ey0) return g;
    g.bx = ex0; g.by = ey0; g.bw = ex1 - ex0; g.bh = ey1 - ey0;
    g.nx = (g.bw / 2 + st - 1) / st; g.ny = (g.bh / 2 + st - 1) / st;
    const int lx = ex0 - cx, ly = ey0 - cy;   // back into the view's frame, then into result coordinates
    g.rect[0] = rot ? vw - (lx + g.bw) : lx; g.rect[1] = rot ? vh - (ly + g.bh) : ly; g.rect[2] = g.bw; g.rect[3] = g.bh;
    return g;
}
constexpr int kMeterWaves = 8, kMeterThreads = 64 * kMeterWaves;
constexpr int kMeterRowsPerBlock = 8;    // a launch takes one partial workgroup per this many rows of the view's frame ...
constexpr int kMeterBlocksMax = 128;     // ... up to this many per frame (one frame alone is latency-bound: it wants every CU) ...
constexpr int kMeterBatchFrames = 4, kMeterBlocksBatch = 32;   // ... and, in a launch of more than 4 frames, up to 32 (the slab's traffic)
constexpr int kMeterLdsBytes = kMeterWaves * 4 * 256 * 4;   // the waves' private [4][256] histograms
inline int meter_blocks(int view_rows, int batch)
{
    const int b = (view_rows + kMeterRowsPerBlock - 1) / kMeterRowsPerBlock, cap = batch > kMeterBatchFrames ? kMeterBlocksBatch : kMeterBlocksMax;
    return b < 1 ? 1 : (b > cap ? cap : b);
}
struct MeterArgs {
    const uint8_t *frames;    // [num_slots][vh][vw][3]: the view's device frames, un-rotated
    size_t frame_bytes;
    const uint8_t *raw;       // [num_slots][raw_h][raw_w] raw CFA frames; nullptr: not a Bayer engine (RAW then meters nothing)
    size_t raw_bytes;
    const MeterParams *params;
    const int2 *win;          // [num_slots] the view's corner in the raw frame (CropArgs::win), read when the kernel runs; nullptr: (0, 0)
    uint32_t *slab;           // [num_slots][kMeterBlocksMax][4][256] partial histograms, rewritten by every launch
    MeterStats *out;          // [batch]: frame b's record, device or pinned
    int first;                // frame b is slot first + b
    int vw, vh, raw_w, raw_h, rotate180, ry, rx;   // ry, rx: parities of the R sites (BayerArgs)
};
// histogram kernel, then the sum of its partials; fast: a lane-group of equal pixels is added once with its sample count
void launch_frame_meter(const MeterArgs &a, int batch, bool fast, hipStream_t s);

// ---- LDS fill / probe (k_debug.hip; test hooks irmv_debug_lds_fill / irmv_debug_lds_probe) ----------------------------
constexpr int kDebugLdsWords = 160 * 1024 / 4;   // the largest LDS allocation of one workgroup on gfx950
int debug_lds_workgroups(int cus);               // several per CU
hipError_t launch_lds_fill(uint32_t pattern, uint32_t *check, int workgroups, hipStream_t s);   // check: one zeroed word, counts read-back mismatches
hipError_t launch_lds_probe(uint32_t pattern, uint32_t word, uint32_t *out, int workgroups, hipStream_t s);   // out: [workgroups][4], zeroed

void launch_pnp_only(const PnpConst &c, const float *pts, int n, int armor_size, double *rvec, double *tvec,
                     int32_t *ok, hipStream_t s);

// ---- constrained pose (k_yaw.hip; irmv_engine_set_yaw_solve) ----------------------------------------------------------
// DevYaw is the side record of one detection (the layout of irmv_yaw_pose).  YawTable and the per-slot YawBasis records live in
// device memory at addresses fixed from the first set_yaw_solve on; the host writes them (engine_yaw.cpp: every unit vector
// and every square root is the host's), the kernel reads them when it runs.
constexpr int kYawRoundsMax = 6, kYawThreads = 256, kYawPerBlock = kYawThreads / 64;
struct DevYaw {
    double rvec[3], tvec[3], quat[4];
    double tau, cs, sn, err;
    int32_t state;            // 0: nothing here (all zero); 1: solved; -1: refused
    int32_t lane[kYawRoundsMax];
    int32_t pad_;
};
struct YawTable {
    int32_t enable, rounds;
    double tau_max;
    double s[kMaxClasses], c[kMaxClasses];   // per class: the tilt n . u and sqrt(1 - s s); c == 0: no basis
};
struct YawBasis { double u[3], h1[3], h2[3]; int32_t ok, pad_; };   // ok == 0: the camera looks along gravity
// What one solve needs of the two tables, as values (the stand-alone form passes it as a kernel argument)
struct YawRule { double u[3], h1[3], h2[3], s, c, tau_max; int32_t rounds, ok; };
struct YawArgs {
    const DevDet *dets;       // [B][max_det]: the records the post stage wrote
    int max_det;
    const int *num_dets;      // frame b: num_dets[b * num_dets_stride]
    int num_dets_stride;
    const PnpConst *pnp;      // frame b solves with pnp[(first + b) * pnp_stride]
    int first, pnp_stride;
    const YawTable *table;
    const YawBasis *basis;    // [num_slots]: frame b's is basis[first + b]
    DevYaw *out;              // [B][max_det]
};
void launch_yaw_solve(const YawArgs &a, int batch, hipStream_t s);
// stand-alone: quad i of pts [n][8] -> out[i], every quad under the one rule
void launch_yaw_points(const PnpConst &c, const float *pts, int n, int armor_size, const YawRule &rule, DevYaw *out, hipStream_t s);

// ---- pose uncertainty (k_posecov.hip; irmv_engine_set_pose_cov) -----------------------------------------------------------
// DevPoseCov is the side record of one detection (the layout of irmv_pose_cov).  PoseCovTable lives in device memory at an
// address fixed from the first set_pose_cov on; the host writes it, the kernel reads it when it runs.
constexpr int kPoseCovN = 21, kPoseCovYawN = 10, kPoseCovSeriesTerms = 16;
struct DevPoseCov {
    double cov[kPoseCovN], chi2, sigma_range;
    double yaw_cov[kPoseCovYawN], yaw_chi2, sigma_yaw;
    int32_t state, yaw_state;   // 0: nothing here (all zero); 1: computed; -1: refused
};
struct PoseCovTable { int32_t enable, pad_; double sigma_px; };
// What the stand-alone form needs beside the camera, as values
struct PoseCovRule { double sigma_px, u[3]; int32_t has_up, pad_; };
struct PoseCovArgs {
    const DevDet *dets;       // [B][max_det]: the records the post stage wrote
    int max_det;
    const int *num_dets;      // frame b: num_dets[b * num_dets_stride]
    int num_dets_stride;
    const PnpConst *pnp;      // frame b's camera is pnp[(first + b) * pnp_stride]
    int first, pnp_stride;
    const PoseCovTable *table;
    const DevYaw *yaw;        // [B][max_det]: where the step's yaw launch wrote its records; nullptr: the engine solves no yaws
    const YawBasis *basis;    // [num_slots]: frame b's up vector is basis[first + b].u (read where yaw is not null)
    DevPoseCov *out;          // [B][max_det]
};
void launch_pose_cov(const PoseCovArgs &a, int batch, hipStream_t s);
// stand-alone: quad i of pts [n][8] with pose poses[i] (rvec, tvec: six doubles) -> out[i]; rule.has_up: the yaw block too
void launch_pose_cov_points(const PnpConst &c, const float *pts, const double *poses, int n, int armor_size, const PoseCovRule &rule,
                            DevPoseCov *out, hipStream_t s);

// ---- armor tracks (k_track.hip; irmv_engine_set_tracking, irmv_tracker) ----------------------------------------------------
// DevDetTrack, DevTrackFrame, DevTrack and TrackObs have the layouts of irmv_det_track, irmv_track_frame, irmv_track and
// irmv_track_obs.  DevTrackTable is the state that outlives a step: one per engine (per stand-alone tracker), read and written
// by track_kernel alone, cleared by the host between steps only.  DevTrackSnap is a slot's record: the header and the table as
// the slot's step left it.  TrackOpts and TrackSlot live in device memory at fixed addresses; the host writes them, the kernel
// reads them when it runs.
constexpr int kTrackCap = 32, kTrackThreads = 256;
constexpr int kTrackClasses = 14;   // IRMV_NUM_CLASSES: a record's class as irmv_det reports it (slot_det)
struct DevDetTrack { int32_t state, track; uint32_t id; int32_t hits; double d2, pos[3], vel[3]; };
struct DevTrackFrame { double stamp; int32_t state, n_live, n_confirmed, n_started, n_deleted, n_no_room; uint32_t next_id; int32_t pad_; };
struct DevTrack {
    uint32_t id;
    int32_t cls, state, hits, misses, det;
    double first, last_hit, stamp;
    double x[6], P[36];
};
struct DevTrackTable { double stamp; int32_t stamped; uint32_t next_id; DevTrack tracks[kTrackCap]; };
struct DevTrackSnap { DevTrackFrame frame; DevTrack tracks[kTrackCap]; };
struct TrackObs { int32_t cls, valid, has_cov, pad_; double tvec[3], cov[9]; };
struct TrackOpts { int32_t enable, confirm_hits, max_misses, match_class; double gate, max_coast_s, accel_sigma, init_vel_sigma, sigma_lat, sigma_rng; };
struct TrackSlot { double stamp, R[9], t[3]; };
struct TrackArgs {
    DevTrackTable *table;
    const TrackOpts *opts;
    const TrackSlot *slots;   // frame b's stamp and camera pose: slots[first + b]
    int first;
    // the engine's form: frame b's records are dets[b * max_det + i], i < min(num_dets[b * num_dets_stride], max_det) ...
    const DevDet *dets;
    int max_det;
    const int *num_dets;
    int num_dets_stride;
    const DevPoseCov *cov;    // ... with their covariances where the step computed them ([B][max_det]); nullptr: the default noise
    // the stand-alone form (dets == nullptr): n_obs <= kMaxDetCap observations of the one frame
    const TrackObs *obs;
    int n_obs;
    DevDetTrack *out_det;     // [B][max_det]: the frame's [0, n) records are written
    DevTrackSnap *out_snap;   // [B]
};
// `batch` frames, one after the other in index order, by ONE workgroup
void launch_track_update(const TrackArgs &a, int batch, hipStream_t s);

// ---- plate patches (k_patch.hip; irmv_engine_set_patches) ---------------------------------------------------------------
// DevPatch is the side record of one detection (the layout of irmv_plate_patch).  PatchTable lives in device memory at an
// address fixed from the first set_patches (or patches_at) on; the host writes it, the kernel reads it when it runs.
constexpr int kPatchW = 20, kPatchH = 28, kPatchN = kPatchW * kPatchH, kPatchWords = kPatchN / 4;
constexpr int kPatchThreads = 256, kPatchPerBlock = kPatchThreads / 64;
constexpr int kPatchSpanMin = 20, kPatchSpanMax = 128, kPatchRowsMax = 28, kPatchTopMax = 27;
struct DevPatch {
    uint32_t gray[kPatchWords];   // [28][20] bytes, row-major: a word is four neighbouring samples of a row
    int32_t state, otsu, n_outside, armor_size;
    uint32_t bar_sum[2], sum;
    int32_t pad_;
};
struct PatchTable { int32_t enable, span[2], light_rows, top, pad_[3]; };
struct PatchArgs {
    const uint8_t *frames;    // [B][H][W][3] device frames, un-rotated (rotation folded into the fetch): LightArgs::frames
    size_t frame_bytes;
    int W, H, rotate180;
    const DevDet *dets;       // [B][max_det]: the records the post stage wrote
    int max_det;
    const int *num_dets;      // frame b: num_dets[b * num_dets_stride]
    int num_dets_stride;
    const PatchTable *table;
    DevPatch *out;            // [B][max_det]
};
void launch_patch_step(const PatchArgs &a, int batch, hipStream_t s);
// on demand: quad i of kpts [n][8] (frame coordinates) with plate sizes[i] on the one frame a.frames -> a.out[i]; a.dets,
// a.num_dets and the table's enable are not read
void launch_patch_points(const PatchArgs &a, const float *kpts, const int32_t *sizes, int n, hipStream_t s);

// ---- plate numbers (k_number.hip; irmv_engine_set_numbers) ----------------------------------------------------------------
// DevNumber is the side record of one detection (the layout of irmv_plate_number).  NumberTable, the fp16 weights and the
// fp32 biases live in device memory at addresses fixed from the first set_number_model on; the host writes them (every value
// checked first), the kernel reads them when it runs.  Layer l: weights k-major [dims[l]][pad[l]] halves at w_off[l], zero
// behind dims[l + 1]; biases [pad[l]] floats at b_off[l].
constexpr int kNumIn = kPatchN, kNumHiddenMax = 128, kNumClassMax = 16, kNumLayersMax = 3, kNumPadUnit = 16;
constexpr int kNumWeightHalves = kNumIn * kNumHiddenMax + kNumHiddenMax * kNumHiddenMax + kNumHiddenMax * kNumClassMax;
constexpr int kNumBiasFloats = 2 * kNumHiddenMax + kNumClassMax;
constexpr int kNumRecWords = 24;
struct DevNumber {
    int32_t state, label, second, ones;
    float margin;
    int32_t pad_[3];
    float logits[kNumClassMax];
};
struct NumberTable {
    int32_t enable, n_layers, input, pad_;
    int32_t dims[4];                       // dims[0] = 560
    int32_t pad[kNumLayersMax], w_off[kNumLayersMax], b_off[kNumLayersMax], pad2_[3];
};
struct NumberArgs {
    const DevPatch *patches;  // [B][max_det]: where the step's patch op wrote them
    int max_det;
    const int *num_dets;      // frame b: num_dets[b * num_dets_stride]
    int num_dets_stride;
    const NumberTable *table;
    const half_t *weights;
    const float *bias;
    DevNumber *out;           // [B][max_det]
};
void launch_number_step(const NumberArgs &a, int batch, hipStream_t s);
// on demand: patch i of a.patches [n] -> a.out[i]; a.num_dets and the table's enable are not read
void launch_number_points(const NumberArgs &a, int n, hipStream_t s);
// both solutions, A first: rvec / tvec [n][2][3], err [n][2], ok bit 0 = launch_pnp_only's ok, bit 1 = B passed its own finiteness check
void launch_pnp_both(const PnpConst &c, const float *pts, int n, int armor_size, double *rvec, double *tvec, double *err,
                     int32_t *ok, hipStream_t s);

}  // namespace irmv
