// libirmv_hip.so host side: engine object, execution plan, hipGraph capture, C ABI.
//
// MI355X-first counterpart of irmv_detection::YoloEngine (reference
// src/yolo_engine.cpp) and PnPSolver (src/pnp_solver.cpp):
//   * frame slots are pinned host memory (hipHostMalloc) copied to HBM by an
//     async copy on a dedicated upload stream, event-chained to the captured
//     step (results need no download: the NMS kernel stores its records straight into mapped pinned host memory;
//     only the classical-extraction mode keeps device records + one D2H copy) -- the dGPU
//     answer to the reference's cudaMallocManaged source buffer (:60-61) +
//     TripleBuffer: slot n+1 uploads while slot n computes;
//   * one set of weights per device shared by all slots (the reference builds
//     three full engines, src/irm_detector.cpp:35-38);
//   * the kernels of a step {front, fused C2f blocks, convs, pool, decode, NMS+PnP}
//     are captured once per (first_slot, count) into a hipGraph (:102-107),
//     and `count` independent frames ride through every kernel as the batch
//     dimension of its GEMM M axis, which is what fills 256 CUs;
//   * no host work between launch and results except the final struct copy
//     (parse_output's scaling, :202-220, runs in the NMS kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <set>
#include <memory>
#include <string>
#include <vector>

#include "../../include/irmv_hip.h"
#include "irmv_common.hpp"
#include "numa.hpp"

using namespace irmv;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(IRMV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

extern "C" const char *irmv_last_error(void) { return g_err.c_str(); }
// "irmv_hip 0.3 (gfx950; HIP runtime <hipRuntimeGetVersion>)": the runtime that actually serves this library.  It is the
// process's FIRST libamdhip64.so.7 -- /opt/rocm's 7.2 on its own, torch's bundled 7.0 (same SONAME) when `import torch`
// came first.
extern "C" const char *irmv_version(void)
{
    static char buf[96];
    static std::once_flag once;
    std::call_once(once, [] {
        int v = 0;
        if (hipRuntimeGetVersion(&v) != hipSuccess) v = 0;
        snprintf(buf, sizeof buf, "irmv_hip 0.3 (gfx950; HIP runtime %d)", v);
    });
    return buf;
}
extern "C" int irmv_device_synchronize(int device)
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    return IRMV_OK;
}
extern "C" int irmv_device_count(int *count)
{
    if (!count) return fail(IRMV_ERR_ARG, "count is null");
    HIP_TRY(hipGetDeviceCount(count));
    return IRMV_OK;
}

// ---- .irmw blob ------------------------------------------------------------------
#pragma pack(push, 1)
struct BlobHeader { char magic[4]; uint32_t version, nc, nk, reg_max, n_layers, dtype, reserved; };
struct BlobLayer { char name[32]; uint32_t cin, cout, k, stride, act, pad; uint64_t w_off, b_off; };
#pragma pack(pop)

struct LayerW {
    std::string name;
    int cin, cout, k, stride, act;
    int groups;         // > 1: depthwise (groups == cout, cin == 1)
    const uint16_t *w;  // OHWI fp16 bits (points into the blob copy)
    const float *b;
};

static float half_bits_to_float(uint16_t h)
{
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, x;
    if (exp == 0) {
        if (man == 0) x = sign;
        else {
            int e = -1;
            do { e++; man <<= 1; } while (!(man & 0x400u));
            x = sign | ((uint32_t)(112 - e) << 23) | ((man & 0x3ffu) << 13);
        }
    } else if (exp == 31) x = sign | 0x7f800000u | (man << 13);
    else x = sign | ((exp + 112u) << 23) | (man << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// float -> IEEE fp16 bits, round to nearest even (dequantised int8 weights are stored as the fp16 the kernels multiply with)
static uint16_t float_to_half_bits(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0u));   // inf / nan
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                          // rounds to inf
    if (x < 0x33000001u) return (uint16_t)sign;                                                        // rounds to zero
    if (x < 0x38800000u) {   // subnormal half
        const int shift = 126 - (int)(x >> 23);                     // 14..24
        const uint32_t man = (x & 0x7fffffu) | 0x800000u;
        uint32_t h = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    uint32_t h = ((x >> 23) - 112u) << 10 | ((x >> 13) & 0x3ffu);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
}

// ---- engine ----------------------------------------------------------------------
struct Tensor {
    std::string name;
    void *base = nullptr;
    size_t slot_elems = 0;
    int H = 0, W = 0, C = 0;
    bool f32 = false;
    size_t esize() const { return f32 ? 4 : 2; }
    void *slot(int s) const { return static_cast<char *>(base) + (size_t)s * slot_elems * esize(); }
};

struct SegRef { int t = -1, coff = 0, C = 0, shift = 0; };

// The environment switches of the tuner, read once per engine: each takes effect for every engine created after it is set.
struct TuneSwitches {
    bool untuned, verbose, warn;        // IRMV_AUTOTUNE=0, IRMV_AUTOTUNE_VERBOSE, IRMV_TUNE_WARN
    bool has_s2, has_wres;              // IRMV_FORCE_S2=lds|ct|deep, IRMV_FORCE_WRES=<n> (parity tests) are set ...
    std::string force_s2, force_wres;   // ... to these values (copies: an engine's hooks read them after the environment may have changed)
    bool force_pw, force_pwn, force_cm, force_w8, force_nt8, force_pf4;
    bool no_pw, no_pwn, no_pf2, no_pf4, no_cm, no_w8, no_nt8, no_wres, no_deep;
};

enum OpKind { OP_PRE, OP_CONV0, OP_CONV, OP_POOL, OP_NMS, OP_LIGHT, OP_FRONT, OP_C2F2, OP_C2F32, OP_DW, OP_SHUF, OP_SCAN, OP_BNECK, OP_KPT3, OP_DEMOSAIC, OP_CROP };

struct Op {
    OpKind kind;
    std::string layer;
    ConvCfg cfg{};      // tile shape for full batched steps (count == num_slots)
    ConvCfg cfg_one{};  // tile shape for single-frame steps (latency mode)
    char kname_one[48] = {0};
    SegRef s0, s1;
    int Hin = 0, Win = 0, Hout = 0, Wout = 0, cin = 0, cout = 0, cout_pad = 0, ksteps = 0;
    int out_t = -1, out_coff = 0, res_t = -1, res_coff = 0;
    half_t *w_packed = nullptr;
    half_t *w_k16 = nullptr;   // 1x1 layers with Cin = 16 and fp32 output (the keypoint branch's finals): the weights in the A layout of v_mfma_f32_16x16x16_f16 [64 lanes][4]
    half_t *w_lds[4] = {nullptr, nullptr, nullptr, nullptr};   // LDS-kernel layout for nt = 1 / 2 / 4 / 8 (eligible 3x3 layers only; nt = 8: stride-2 layers with >= 128 output channels)
    float *bias = nullptr;
    double flops = 0, bytes = 0;  // per frame (bytes: activations in + out, plus the weights)
    double w_bytes = 0;           // the weights' share of `bytes`: read once per LAUNCH, not once per frame (irmv_engine_profile)
    double out_bytes = 0;         // the output's share (a conv that carries a fused 1x1 writes that layer's output instead of its own)
    bool pair = false;
    int level = -1;    // Detect level of a head op (-1: trunk)
    char kname[48] = {0};
    int sub[4] = {-1, -1, -1, -1};   // OP_C2F2 / OP_C2F32: indices of the layer ops whose weights it uses
    int mode = 0;                    // OP_C2F32: 0 whole block, 1 cv1 + first bottleneck, 2 last bottleneck + cv2
    bool shortcut = false;
    int fuse_next = -1;        // LDS 3x3 conv: index of the 1x1 op computed in its epilogue (Detect-head finals), -1 = none
    bool fused_away = false;   // preprocess / model.0 / model.1 when the fused front kernel runs them (kept for read-backs)
    int group = -1;            // single-frame steps: index into irmv_engine::head_groups of the one launch this conv rides in
    int bneck = -1;            // single-frame steps: index of the OP_BNECK launch (k_bneck.hip) that computes this conv; OP_BNECK itself: 1 = kept
    int kpt3 = -1;             // a keypoint-branch conv: index of the OP_KPT3 launch (k_kpt.hip) that computes its level's branch in every step; OP_KPT3 itself: 1
    bool gated_first = false;  // a Detect box branch's first conv that some step runs behind the tile gate (sparse branch): its tensor is lazy, the read-back step runs it densely
    int tune_fuse[2] = {-1, -1};   // OP_CONV: fuse_next as the autotuner's two passes (stream share, one slot) found it (test hooks rebuild their candidate lists)
};

// What a step launches depends only on its kind and the engine, so each kind's launch list is decided at creation (build_step_plans).
// BATCH: count > 1 slots; ONE: one slot; MATERIALIZE: the layers fused kernels keep on chip (read-backs); POST: run_post's kernels.
enum StepKind { STEP_BATCH, STEP_ONE, STEP_MATERIALIZE, STEP_POST };

struct Launch {
    int op = -1, group = -1;  // index into irmv_engine::ops; >= 0: the head group (head_groups) launched at its first member's place
    bool cfg_one = false;     // OP_CONV: runs op.cfg_one, not op.cfg
    bool fused = false;       // OP_CONV: carries its fuse_next 1x1 in the epilogue
    unsigned scan = 0;        // bit k: member k of the group (a lone conv: bit 0) appends scan candidates from its epilogue
    bool keys_only = false;   // OP_NMS: decodes the boxes of its key lists itself
    bool sparse = false;      // a Detect box carrier or OP_KPT3 behind its level's class carrier: stores the candidate anchors' head rows only
    int gate = 0;             // sparse branch, ConvArgs::tile_gate / Kpt3Args::tile_gate: 0 = off, 1 = halo 0 (writes head rows), 2 = halo 1 (box branch's first conv)
    bool once = false;        // not repeated under irmv_engine_profile (appends to, consumes or rewrites per-frame lists)
    std::string name, layer;  // irmv_engine_profile's row
    double flops = 0, bytes = 0, launch_bytes = 0;   // per frame; launch_bytes (the weights): once per launch
};

struct GraphKey {
    int first, count;
    StepKind kind;
    bool upload;   // the frames' upload is the graph's first node
    bool operator<(const GraphKey &o) const { return std::tie(first, count, kind, upload) < std::tie(o.first, o.count, o.kind, o.upload); }
};

// Events of one submitted slot group [first, first + count): h2d = its frames are in HBM (async upload only);
// out = its kernels have run and its results are host-visible (so its device frames may be overwritten too).
struct SlotGroup {
    int first = 0, count = 0;
    hipEvent_t h2d = nullptr, out = nullptr;
    hipStream_t compute = nullptr;   // compute stream of the last submit
    bool in_flight = false;          // submitted and not yet known complete
    bool async_up = false;           // the last submit uploaded on the side stream (event h2d is valid)
};

struct irmv_engine {
    irmv_engine_cfg cfg{};
    int nc = 0, nk = 0, A = 0, no = 0;
    int backbone = 0;   // 0: C2f stages (YOLOv8n), 1: ShuffleNetV2 stages (blob header)
    int num_cus = 256;  // compute units of the device (persistent kernels size their grids by it)
    int numa_node = -1;     // host NUMA node closest to the device (hipDeviceAttributeHostNumaId); -1: unknown
    bool numa_placed = false;   // the pinned frame slots were allocated and first touched under that node's CPU set and memory policy
    // Single-frame engines: the independent Detect-branch convs of the three levels as one launch per stage (k_conv.hip
    // conv3x3_lds_multi / conv_mfma_multi).  family 0: LDS 3x3 with tile (mt 1, nt); 1: direct kernel with cfg.
    struct HeadGroup { std::vector<int> members; int family = 0, nt = 1; ConvCfg cfg{}; char name[48] = {0}; };
    std::vector<HeadGroup> head_groups;
    bool post_keys_only = false;   // IRMV_POST_KEYS_ONLY=1 (tests): run_post's NMS ignores scan_decode_kernel's boxes and decodes its own, as a whole step's does
    bool emit_scan = false;   // candidates are emitted by the class-branch conv epilogues (needs split_scan's counters and all three levels fused)
    bool split_scan = true;   // scan + box decode as a multi-workgroup kernel in front of nms_pnp (IRMV_SPLIT_SCAN=0: inside it)
    int *cand_counts = nullptr;
    // Sparse head: a step stores the head rows of candidate anchors only (the one reader, nms_pnp_kernel, reads no others).
    // The class carriers set a bit per candidate anchor, box carriers and OP_KPT3 store where it is set, nms_pnp_kernel clears
    // it again.  Needs emit_scan; IRMV_SPARSE_HEAD=0: every row is stored.  head_stale[slot]: the slot's head in memory is
    // the sparse one of its last step -- whatever reads it runs the read-back step first (ensure_dense_head).
    bool sparse_head = false;
    unsigned int *cand_bits = nullptr;   // [S][cand_words], zero between steps
    int cand_words = 0;
    std::vector<char> head_stale;
    // Sparse branch (IRMV_SPARSE_BRANCH=0: off; only with sparse_head): the launches behind the class carriers also skip the
    // COMPUTATION of (tile, image) pairs without a candidate anchor (Launch::gate).  The box branch's gated first conv leaves its
    // tensor stale outside active tiles: branch_stale[slot], until the read-back step has run it densely.
    bool sparse_branch = false;
    std::vector<char> branch_stale;
    int lvl_hw[3] = {0, 0, 0}, lvl_base[3] = {0, 0, 0};
    size_t frame_bytes = 0;       // one HWC source frame (src_dev, rot_dev)
    size_t src_bytes = 0;         // one source slot as the producer writes it (src_host, and raw_dev or src_dev): frame_bytes, or W*H for a Bayer engine
    hipStream_t stream = nullptr;                 // stream 0: single-slot detect(), read-backs, profile
    hipStream_t extra_streams[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // streams 1..num_streams-1
    int num_streams = 1;
    // frame hand-off: uploads can ride a stream of their own, chained to the compute streams by the
    // events of the submitted slot group
    hipStream_t h2d_stream = nullptr;
    std::map<std::pair<int, int>, SlotGroup> groups;   // (first, count) -> events of that group's last submit
    std::vector<SlotGroup *> slot_owner;               // per slot: the group whose submit touched it last
    bool inline_copies = false;                        // IRMV_INLINE_COPIES=1: round-1 behaviour, copies on the compute stream
    bool graph_upload = true;                          // uploads that ride the compute stream are a node of the step's graph (IRMV_GRAPH_UPLOAD=0: a separate launch in front of it; measured
                                                       // again in round 5 with the upload kernel: 0.3365 - 0.3438 ms against 0.335 - 0.336 as the first node: no hiding of the graph's launch cost)
    uint8_t *src_host = nullptr;  // pinned [S][frame]
    int sync_launch = 0;               // how a synchronous single-frame step (detect()) reaches the GPU: 0 = one hipGraph replay (upload = its first node), 1 = launched
                                       // kernel by kernel behind the upload; chosen by timing at creation (choose_sync_launch), IRMV_SYNC_LAUNCH=graph|eager forces
    uint8_t *src_host_dev = nullptr;   // the same memory through the device's mapping (the upload kernel reads it: launch_upload_frames)
    int upload_kernel_blocks = 256;    // 0: synchronous single-frame uploads ride the copy engine like every other upload (IRMV_UPLOAD_KERNEL=0)
    uint8_t *src_dev = nullptr;   // [S][frame]
    uint8_t *raw_dev = nullptr;   // Bayer engines: [S][W*H] raw frames, demosaiced into src_dev by the first op of a step (OP_DEMOSAIC)
    BayerArgs bayer{};            // (pointers, slot strides, pattern phase and gains of that op; raw / dst set per launch)
    // The ISP table of a Bayer engine (irmv_engine_set_bayer_isp): gains and tone LUT folded into T[c][v], [3][256] bytes in
    // device memory, read by the table kernels when they run -- a captured graph holds the pointer, never the values.
    // bayer_table: the demosaic is a table kernel (an MHC engine from creation on, a bilinear one from its first set).
    uint8_t *isp_table_dev = nullptr;
    bool bayer_table = false, bayer_mhc = false;
    uint16_t isp_gain[3] = {256, 256, 256};
    uint8_t isp_lut[kBayerTableBytes] = {0};
    uint8_t *rot_dev = nullptr;   // [frame]
    // Tracking window (irmv_engine_cfg.win_width / win_height): cfg.src_width x cfg.src_height is then the WINDOW -- what every
    // kernel behind the crop sees as its source frame -- and full_w x full_h the frame the producer writes.  OP_CROP cuts the
    // window at win_dev[slot] out of the slot's full frame (full_dev, or the pinned slot itself) into its src_dev frame.
    // Without a window full_w x full_h equals the cfg's source size and none of the rest exists.
    bool window = false;
    int full_w = 0, full_h = 0;
    size_t full_bytes = 0;            // one full HWC frame (full_dev)
    uint8_t *full_dev = nullptr;      // [S][full frame]: what an HWC window engine's uploads and a Bayer one's demosaic write
    int2 *win_dev = nullptr;          // [S] the windows' corners in buffer coordinates, read by window_crop_kernel when it runs
    std::vector<int2> win_org;        // [S] the corners as set, in result coordinates (the rotated frame under rotate180)
    std::vector<int2> sub_org;        // [S] ... as they were at the slot's last submit: what its results are shifted by
    bool window_upload = true;        // synchronous steps of one or two slots crop straight out of the pinned slot (IRMV_WINDOW_UPLOAD=0: upload, then crop)
    PnpConst pnp_base{};              // the camera as configured; pnp_dev[slot] = pnp_base with the principal point moved by the slot's corner
    AxisTap *tap_x = nullptr, *tap_y = nullptr;
    std::vector<Tensor> tensors;
    std::map<std::string, int> tensor_idx;
    std::vector<Op> ops;
    std::vector<Launch> plans[STEP_POST + 1];   // per StepKind: the launches of such a step, in order (build_step_plans)
    std::vector<void *> dev_allocs;
    int head_t[3] = {-1, -1, -1};
    float *head_all = nullptr;
    PnpConst *pnp_dev = nullptr;
    long long *dbg_dev = nullptr;
    std::set<std::string> lazy_tensors;   // tensors a step does not write because a fused kernel keeps them on chip
    bool fused_front = false;          // OP_FRONT replaces preprocess + model.0.conv + model.1.conv in a step
    int front_tiles_x = 0, front_tiles_y = 0, front_stage_bytes = 0, front_tile_y = kFrontTileY;
    int front_v[4] = {0, 0, 0, 0};     // valid (non-padding) net-input column / row ranges
    int front_fastx = 0, front_fx_i0 = 0, front_fx_step = 2;   // every x tap is (i0 + 2 k, i0 + 2 k + 1; 1/2): the front kernel's 2 : 1 column path
    bool classical = false;            // four points from the classical light extraction instead of a keypoint head
    signed char *light_labels = nullptr;   // label pool: light_pool bytes per slot
    size_t light_pool = 0;
    short *light_points = nullptr, *light_hulls = nullptr;
    float *light_boxes = nullptr;      // explicit boxes of irmv_engine_extract_armors
    DevDet *light_dets_dev = nullptr, *light_dets_host = nullptr;
    LightTrace *light_trace_dev = nullptr;   // [max_det], allocated by the first irmv_engine_light_trace
    float *boxes = nullptr;
    unsigned long long *keys = nullptr;
    DevDet *dets_dev = nullptr, *dets_host = nullptr, *dets_host_dev = nullptr;       // *_host_dev: device view of the pinned buffer
    DevFrameOut *fout_dev = nullptr, *fout_host = nullptr, *fout_host_dev = nullptr;
    bool zero_copy_results = false;   // the NMS kernel writes its results straight into pinned host memory (no D2H copy)
    half_t *conv0_w = nullptr;
    float *conv0_b = nullptr;
    PostArgs post{};
    std::map<GraphKey, hipGraphExec_t> graphs;
    double last_detect_ms = 0;
    std::vector<uint8_t> blob;
    std::vector<LayerW> layers;
    std::vector<std::vector<uint16_t>> dequant;   // int8 blobs: per layer fp16(q * scale), what LayerW::w points to
    std::vector<std::vector<uint16_t>> merged_w;  // Detect first-stage convs of a level concatenated along cout (single-frame engines)
    std::vector<std::vector<float>> merged_b;
    bool bneck64 = true;       // single-frame steps run the 64-channel Bottlenecks of the C2f blocks (and their cv2) as one launch each (IRMV_BNECK64=0: off)
    bool merge_head0 = false;
    bool kpt3 = true;          // the keypoint branch of a Detect level as one launch (engines that do not merge the first-stage Detect convs; IRMV_KPT3=0: off)
    TuneSwitches tune_sw{};    // the tuner's switches as autotune_convs read them (the conv test hooks list the same candidates)

    ~irmv_engine();
};

// Optional allocation log (IRMV_LOG_ALLOC=1): every device / pinned range an engine owns, so that a faulting
// address reported by the driver can be mapped to a buffer.
static bool log_alloc() { static const bool on = getenv("IRMV_LOG_ALLOC") != nullptr; return on; }
static void log_range(const irmv_engine *e, const char *what, const void *p, size_t bytes)
{
    if (log_alloc()) fprintf(stderr, "[irmv alloc] engine %p %-18s [%p, %p) %zu bytes\n", (const void *)e, what, p, (const void *)((const char *)p + bytes), bytes);
}

// Teardown order matters: nothing may be freed while any stream of this engine can still touch it.
//   1. drain EVERY stream the engine ever enqueued work on (compute, upload, download, capture side lanes);
//   2. destroy the graph executables (they hold kernel-argument copies pointing into the buffers);
//   3. free device memory, then pinned host memory;
//   4. destroy events and streams.
irmv_engine::~irmv_engine()
{
    if (cfg.device >= 0) (void)hipSetDevice(cfg.device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (int i = 0; i < 7; i++)
        if (extra_streams[i]) (void)hipStreamSynchronize(extra_streams[i]);
    if (h2d_stream) (void)hipStreamSynchronize(h2d_stream);
    if (dbg_dev) {   // diagnostic: phase cycles of the last nms_pnp launch per slot (100 MHz s_memtime-independent clock64)
        std::vector<long long> h((size_t)cfg.num_slots * 16);
        if (hipMemcpy(h.data(), dbg_dev, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
            for (int s = 0; s < cfg.num_slots && s < std::max(4, atoi(getenv("IRMV_NMS_STAMPS") ? getenv("IRMV_NMS_STAMPS") : "0")); s++)   // IRMV_NMS_STAMPS=<n>: the first n slots (at least four)
            {
                const long long *t = &h[(size_t)s * 16];
                fprintf(stderr, "[nms stamps] slot %d: keys %lld select %lld decode %lld sort %lld gather+classes %lld rows %lld walk %lld kpts %lld pnp %lld store %lld cycles; total %lld; n=%lld kept=%lld\n", s,
                        t[7] - t[0], t[8] - t[7], t[9] - t[8], t[1] - t[9], t[10] - t[1], t[2] - t[10], t[3] - t[2], t[11] - t[3], t[12] - t[11], t[4] - t[12], t[4] - t[0], t[5], t[6]);
            }
    }
    for (auto &g : graphs) (void)hipGraphExecDestroy(g.second);
    graphs.clear();
    if (log_alloc()) fprintf(stderr, "[irmv alloc] engine %p destroy: freeing %zu device ranges\n", (const void *)this, dev_allocs.size());
    for (void *p : dev_allocs) (void)hipFree(p);
    dev_allocs.clear();
    if (src_host) (void)hipHostFree(src_host);
    if (dets_host) (void)hipHostFree(dets_host);
    if (fout_host) (void)hipHostFree(fout_host);
    if (light_dets_host) (void)hipHostFree(light_dets_host);
    for (auto &kv : groups) {
        if (kv.second.h2d) (void)hipEventDestroy(kv.second.h2d);
        if (kv.second.out) (void)hipEventDestroy(kv.second.out);
    }
    for (int i = 0; i < 7; i++)
        if (extra_streams[i]) (void)hipStreamDestroy(extra_streams[i]);
    if (h2d_stream) (void)hipStreamDestroy(h2d_stream);
    if (stream) (void)hipStreamDestroy(stream);
}

// slots handled by one stream of a multi-slot submit
static int stream_share(const irmv_engine *e, int count) { return (count + e->num_streams - 1) / e->num_streams; }

static int dev_alloc(irmv_engine *e, void **p, size_t bytes)
{
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    e->dev_allocs.push_back(*p);
    log_range(e, "device", *p, bytes ? bytes : 16);
    return IRMV_OK;
}

static int new_tensor(irmv_engine *e, const std::string &name, int H, int W, int C, bool f32, int *idx)
{
    Tensor t;
    t.name = name;
    t.H = H; t.W = W; t.C = C; t.f32 = f32;
    t.slot_elems = (size_t)H * W * C;
    int rc = dev_alloc(e, &t.base, t.slot_elems * t.esize() * e->cfg.num_slots);
    if (rc) return rc;
    // activations start at zero so that never-written pad channels are finite
    HIP_TRY(hipMemset(t.base, 0, t.slot_elems * t.esize() * e->cfg.num_slots));
    *idx = (int)e->tensors.size();
    e->tensor_idx[name] = *idx;
    e->tensors.push_back(t);
    return IRMV_OK;
}

static const LayerW *find_layer(const irmv_engine *e, const std::string &name)
{
    for (auto &l : e->layers)
        if (l.name == name) return &l;
    return nullptr;
}

// output channel held by row p of 16-row MFMA tile t (see k_conv.hip epilogue)
static int tile_row_cout(int t, int p, bool pair)
{
    if (!pair) return t * 16 + p;
    return (t >> 1) * 32 + (p >> 2) * 8 + (t & 1) * 4 + (p & 3);
}

static int pack_conv(irmv_engine *e, const LayerW &l, Op &op)
{
    const int taps = l.k * l.k;
    op.cout_pad = (l.cout + 15) / 16 * 16;
    const int ntiles = op.cout_pad / 16;
    const bool pair = !op.cfg.out_f32 && (op.cout_pad % 32 == 0);   // independent of the tile shape chosen later
    op.pair = pair;
    const int cpt = (l.cin + 31) / 32;
    op.ksteps = op.cfg.cin16 ? (taps + 1) / 2 : taps * cpt;
    std::vector<uint16_t> packed((size_t)ntiles * op.ksteps * 512, 0);
    for (int t = 0; t < ntiles; t++)
        for (int ks = 0; ks < op.ksteps; ks++)
            for (int lane = 0; lane < 64; lane++) {
                const int g = lane >> 4, r = lane & 15;
                const int co = tile_row_cout(t, r, pair);
                for (int j = 0; j < 8; j++) {
                    int tap, c;
                    if (op.cfg.cin16) { tap = 2 * ks + (g >> 1); c = 8 * (g & 1) + j; }
                    else { tap = ks / cpt; c = (ks % cpt) * 32 + 8 * g + j; }
                    uint16_t v = 0;
                    if (co < l.cout && tap < taps && c < l.cin) v = l.w[((size_t)co * taps + tap) * l.cin + c];
                    packed[(((size_t)t * op.ksteps + ks) * 64 + lane) * 8 + j] = v;
                }
            }
    // SiLU layers compute on log2 e-scaled activations (irmv_common.hpp, "activation scale"): weights as they are, the bias
    // scaled once here; layers without activation (the Detect finals) undo the scale in their epilogue and keep their bias
    std::vector<float> bias(op.cout_pad, 0.f);
    for (int i = 0; i < l.cout; i++) bias[i] = l.act == 1 ? (float)((double)l.b[i] * (double)kActScale) : l.b[i];
    int rc = dev_alloc(e, (void **)&op.w_packed, packed.size() * 2);
    if (rc) return rc;
    rc = dev_alloc(e, (void **)&op.bias, bias.size() * 4);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(op.w_packed, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(op.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    if (l.k == 1 && l.cin == 16 && op.cfg.out_f32 && l.act == 0 && op.cout_pad == 16) {   // lane (g, r): output channel r, input channels 4 g .. 4 g + 3
        std::vector<uint16_t> pk(64 * 4, 0);
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++)
                if ((lane & 15) < l.cout) pk[lane * 4 + j] = l.w[(size_t)(lane & 15) * l.cin + 4 * (lane >> 4) + j];
        int rc3 = dev_alloc(e, (void **)&op.w_k16, pk.size() * 2);
        if (rc3) return rc3;
        HIP_TRY(hipMemcpy(op.w_k16, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    }
    // LDS-kernel layout: [n-block][chunk of 32 ch][tap][tile in block][lane][8]
    if (l.k == 3 && l.cin % 32 == 0 && l.act == 1 && !op.cfg.out_f32) {
        const int chunks = l.cin / 32;
        for (int v = 0; v < 4; v++) {
            const int nt = 1 << v;
            if (ntiles % nt != 0 || (nt > 1 && !pair)) continue;
            if (nt == 8 && l.stride != 2) continue;      // the 128-channel workgroup exists for the stride-2 layers only (k_conv.hip)
            std::vector<uint16_t> pl((size_t)ntiles * chunks * 9 * 512, 0);
            for (int t = 0; t < ntiles; t++)
                for (int ch = 0; ch < chunks; ch++)
                    for (int tap = 0; tap < 9; tap++)
                        for (int lane = 0; lane < 64; lane++) {
                            const int g = lane >> 4, r = lane & 15;
                            const int co = tile_row_cout(t, r, pair);
                            const int nb = t / nt, ti = t % nt;
                            const size_t base = ((((size_t)nb * chunks + ch) * 9 + tap) * nt + ti) * 512 + (size_t)lane * 8;
                            for (int j = 0; j < 8; j++) {
                                const int c = ch * 32 + 8 * g + j;
                                if (co < l.cout) pl[base + j] = l.w[((size_t)co * 9 + tap) * l.cin + c];
                            }
                        }
            int rc2 = dev_alloc(e, (void **)&op.w_lds[v], pl.size() * 2);
            if (rc2) return rc2;
            HIP_TRY(hipMemcpy(op.w_lds[v], pl.data(), pl.size() * 2, hipMemcpyHostToDevice));
        }
    }
    return IRMV_OK;
}

static int add_conv(irmv_engine *e, const std::string &layer, SegRef s0, SegRef s1, int Hin, int Win, int out_t,
                    int out_coff, int res_t = -1, int res_coff = 0)
{
    const LayerW *l = find_layer(e, layer);
    if (!l) return fail(IRMV_ERR_MODEL, "weight blob has no layer " + layer);
    if (l->cin != s0.C + s1.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": cin does not match the graph");
    Op op;
    op.kind = OP_CONV;
    op.layer = layer;
    op.s0 = s0; op.s1 = s1;
    op.Hin = Hin; op.Win = Win;
    op.Hout = Hin / l->stride; op.Wout = Win / l->stride;
    op.cin = l->cin; op.cout = l->cout;
    op.out_t = out_t; op.out_coff = out_coff; op.res_t = res_t; op.res_coff = res_coff;
    const Tensor &ot = e->tensors[out_t];
    if (ot.H != op.Hout || ot.W != op.Wout) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output shape mismatch");
    const int cout_pad = (l->cout + 15) / 16 * 16;
    if (out_coff + cout_pad > ot.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output slice out of range");
    op.cfg.ks = l->k; op.cfg.stride = l->stride; op.cfg.act = l->act; op.cfg.out_f32 = ot.f32;
    op.cfg.cin16 = (l->cin == 16 && l->k == 3);
    op.cfg.lds = false;
    op.cfg.ipw = 1;
    const int nt_all = cout_pad / 16;
    op.cfg.nt = nt_all >= 4 ? 4 : nt_all;
    // enough workgroups to cover 256 CUs a few times, else halve the pixel tile
    const long m_batch = (long)e->cfg.num_slots * op.Hout * op.Wout;
    const long blocks_mt2 = ((m_batch + 127) / 128) * (cout_pad / (16 * op.cfg.nt));
    op.cfg.mt = blocks_mt2 >= 512 ? 2 : 1;
    op.cfg_one = op.cfg;
    op.cfg_one.mt = 1;
    conv_cfg_name(op.cfg, op.kname, sizeof op.kname);
    conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one);
    op.flops = 2.0 * op.Hout * op.Wout * (double)l->cout * l->cin * l->k * l->k;
    // algorithmic bytes: every input element once (a half-resolution segment = the tensor that exists, not its upsampled
    // image), the output once, the weights once
    op.bytes = 2.0 * ((double)(Hin >> s0.shift) * (Win >> s0.shift) * s0.C + (double)(Hin >> s1.shift) * (Win >> s1.shift) * s1.C) +
               (double)op.Hout * op.Wout * l->cout * (ot.f32 ? 4.0 : 2.0) + 2.0 * l->cout * l->cin * l->k * l->k;
    op.w_bytes = 2.0 * l->cout * l->cin * l->k * l->k;
    op.out_bytes = (double)op.Hout * op.Wout * l->cout * (ot.f32 ? 4.0 : 2.0);
    int rc = pack_conv(e, *l, op);
    if (rc) return rc;
    e->ops.push_back(op);
    return IRMV_OK;
}

#define TRY(x)            \
    do {                  \
        int _rc = (x);    \
        if (_rc) return _rc; \
    } while (0)

// Depthwise 3x3 (ShuffleNetV2 stages): weights repacked tap-major [9][C] so that a lane's 8 channels are one 16-byte load
static int add_dw(irmv_engine *e, const std::string &layer, SegRef in, int Hin, int Win, int out_t, int out_coff)
{
    const LayerW *l = find_layer(e, layer);
    if (!l) return fail(IRMV_ERR_MODEL, "weight blob has no layer " + layer);
    if (l->groups != l->cout || l->cout != in.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": not a depthwise conv over the graph's channels");
    Op op;
    op.kind = OP_DW;
    op.layer = layer;
    op.s0 = in;
    op.Hin = Hin; op.Win = Win; op.Hout = Hin / l->stride; op.Wout = Win / l->stride;
    op.cin = op.cout = op.cout_pad = l->cout;
    op.cfg.stride = l->stride;
    op.out_t = out_t; op.out_coff = out_coff;
    const Tensor &ot = e->tensors[out_t];
    if (ot.H != op.Hout || ot.W != op.Wout || out_coff + l->cout > ot.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output shape mismatch");
    std::vector<uint16_t> w((size_t)9 * l->cout);
    for (int c = 0; c < l->cout; c++)
        for (int t = 0; t < 9; t++) w[(size_t)t * l->cout + c] = l->w[(size_t)c * 9 + t];
    TRY(dev_alloc(e, (void **)&op.w_packed, w.size() * 2));
    TRY(dev_alloc(e, (void **)&op.bias, (size_t)l->cout * 4));
    HIP_TRY(hipMemcpy(op.w_packed, w.data(), w.size() * 2, hipMemcpyHostToDevice));
    {   // no activation, but the output feeds further layers: it stays at the activation scale, so the bias is scaled too
        std::vector<float> bs((size_t)l->cout);
        for (int i = 0; i < l->cout; i++) bs[i] = (float)((double)l->b[i] * (double)kActScale);
        HIP_TRY(hipMemcpy(op.bias, bs.data(), bs.size() * 4, hipMemcpyHostToDevice));
    }
    snprintf(op.kname, sizeof op.kname, "dwconv3x3s%d", l->stride);
    op.flops = 2.0 * op.Hout * op.Wout * (double)l->cout * 9;
    op.bytes = 2.0 * ((double)Hin * Win + (double)op.Hout * op.Wout) * l->cout + 2.0 * 9 * l->cout;
    e->ops.push_back(op);
    return IRMV_OK;
}

// concat + channel shuffle (two groups) of two bc-channel slices: out[2 i] = a[i], out[2 i + 1] = b[i]
static int add_shuffle(irmv_engine *e, const std::string &name, SegRef a, SegRef b, int H, int W, int out_t)
{
    const Tensor &ot = e->tensors[out_t];
    if (a.C != b.C || a.C % 4 != 0 || ot.C != 2 * a.C || ot.H != H || ot.W != W) return fail(IRMV_ERR_MODEL, name + ": shuffle shapes do not match");
    Op op;
    op.kind = OP_SHUF;
    op.layer = name;
    op.s0 = a; op.s1 = b;
    op.Hin = op.Hout = H; op.Win = op.Wout = W;
    op.cin = op.cout = 2 * a.C;
    op.out_t = out_t;
    snprintf(op.kname, sizeof op.kname, "shuffle_cat");
    op.bytes = 2.0 * 2.0 * (double)H * W * 2 * a.C;
    e->ops.push_back(op);
    return IRMV_OK;
}

// ShuffleNetV2 blocks (irmv_detection_amd/arch.py _shuffle_down / _shuffle_unit; the oracle's shuffle_down / shuffle_unit)
static int add_shuffle_down(irmv_engine *e, const std::string &prefix, int in_t, int c1, int H, int W, int c2, int out_t)
{
    const int bc = c2 / 2, Ho = H / 2, Wo = W / 2;
    int d1, b1, p1, d2, b2;
    TRY(new_tensor(e, prefix + ".b1.dw", Ho, Wo, c1, false, &d1));
    TRY(new_tensor(e, prefix + ".b1", Ho, Wo, bc, false, &b1));
    TRY(new_tensor(e, prefix + ".b2.pw1", H, W, bc, false, &p1));
    TRY(new_tensor(e, prefix + ".b2.dw", Ho, Wo, bc, false, &d2));
    TRY(new_tensor(e, prefix + ".b2", Ho, Wo, bc, false, &b2));
    TRY(add_dw(e, prefix + ".b1.dw", SegRef{in_t, 0, c1, 0}, H, W, d1, 0));
    TRY(add_conv(e, prefix + ".b1.pw", SegRef{d1, 0, c1, 0}, SegRef{}, Ho, Wo, b1, 0));
    TRY(add_conv(e, prefix + ".b2.pw1", SegRef{in_t, 0, c1, 0}, SegRef{}, H, W, p1, 0));
    TRY(add_dw(e, prefix + ".b2.dw", SegRef{p1, 0, bc, 0}, H, W, d2, 0));
    TRY(add_conv(e, prefix + ".b2.pw2", SegRef{d2, 0, bc, 0}, SegRef{}, Ho, Wo, b2, 0));
    return add_shuffle(e, prefix + ".shuffle", SegRef{b1, 0, bc, 0}, SegRef{b2, 0, bc, 0}, Ho, Wo, out_t);
}

static int add_shuffle_unit(irmv_engine *e, const std::string &prefix, int in_t, int c, int H, int W, int out_t)
{
    const int bc = c / 2;
    int p1, d2, b2;
    TRY(new_tensor(e, prefix + ".b2.pw1", H, W, bc, false, &p1));
    TRY(new_tensor(e, prefix + ".b2.dw", H, W, bc, false, &d2));
    TRY(new_tensor(e, prefix + ".b2", H, W, bc, false, &b2));
    TRY(add_conv(e, prefix + ".b2.pw1", SegRef{in_t, bc, bc, 0}, SegRef{}, H, W, p1, 0));
    TRY(add_dw(e, prefix + ".b2.dw", SegRef{p1, 0, bc, 0}, H, W, d2, 0));
    TRY(add_conv(e, prefix + ".b2.pw2", SegRef{d2, 0, bc, 0}, SegRef{}, H, W, b2, 0));
    return add_shuffle(e, prefix + ".shuffle", SegRef{in_t, 0, bc, 0}, SegRef{b2, 0, bc, 0}, H, W, out_t);
}

// A C2f block with a 32-channel hidden width (model.4 / model.15 at a 640 net) runs as fused kernels (k_c2f.hip) when its
// layers have the shapes those kernels are written for: n = 1 -> one launch, n = 2 -> two.  The layer ops stay in the
// list as `fused_away` (read-backs of the block's internal tensors run them; they are also the bit-exactness reference).
static int fuse_c2f32(irmv_engine *e, const std::string &prefix, int n, bool shortcut, int cat, int tmp, int out_t)
{
    if (const char *ff = getenv("IRMV_FUSED_C2F")) if (ff[0] == '0') return IRMV_OK;
    const int last = (int)e->ops.size() - 1, first = last - (2 * n + 1);
    if (n < 1 || n > 2 || first < 0) return IRMV_OK;
    const Op &c1 = e->ops[first], &c2 = e->ops[last];
    bool ok = c1.cfg.ks == 1 && c1.cout == 64 && c1.pair && c1.cin % 32 == 0 && c1.s0.C % 32 == 0 && c1.cfg.act == 1 &&
              (c1.ksteps == 2 || c1.ksteps == 4 || c1.ksteps == 6) && (n == 1 || shortcut) &&
              c2.cfg.ks == 1 && c2.cout == 64 && c2.pair && c2.cin == (2 + n) * 32 && c2.ksteps == 2 + n && c2.cfg.act == 1 && !c2.cfg.out_f32;
    for (int i = first + 1; i < last && ok; i++) {
        const Op &m = e->ops[i];
        ok = m.cfg.ks == 3 && m.cfg.stride == 1 && m.cin == 32 && m.cout == 32 && m.pair && m.ksteps == 9 && m.cfg.act == 1 && !m.cfg.cin16;
    }
    if (!ok) return IRMV_OK;
    const int bH = c1.Hin, bW = c1.Win;          // (copies: the pushes below may move e->ops)
    const double c1_bytes = c1.bytes, c1_w = c1.w_bytes;
    auto make = [&](int mode, int i_cv1, int i_m1, int i_m2, int i_cv2, const char *nm) {
        Op op;
        op.kind = OP_C2F32;
        op.mode = mode;
        op.shortcut = shortcut;
        op.layer = prefix + (mode == 0 ? " (fused)" : (mode == 1 ? " (cv1+m.0)" : " (m.1+cv2)"));
        snprintf(op.kname, sizeof op.kname, "%s", nm);
        op.sub[0] = i_cv1; op.sub[1] = i_m1; op.sub[2] = i_m2; op.sub[3] = i_cv2;
        op.Hin = bH; op.Win = bW;
        op.out_t = out_t;
        op.res_t = cat;                              // the block's concat buffer
        const double px = (double)bH * bW;
        for (int k = 0; k < 4; k++)
            if (op.sub[k] >= 0) { op.flops += e->ops[op.sub[k]].flops; e->ops[op.sub[k]].fused_away = true; op.w_bytes += e->ops[op.sub[k]].w_bytes; }
        // algorithmic bytes: block input once (mode 0 / 1), concat slices written / read, block output, every fused layer's weights
        op.bytes = op.w_bytes;
        if (mode != 2) op.bytes += c1_bytes - c1_w - px * 64 * 2.0;                // cv1's inputs
        if (mode == 1) op.bytes += px * 96 * 2.0;                                   // y0 | y1 | y2 written
        if (mode == 2) op.bytes += px * 96 * 2.0;                                   // read back
        if (mode != 1) op.bytes += px * 64 * 2.0;                                   // block output
        e->ops.push_back(op);
    };
    if (n == 1) make(0, first, first + 1, first + 2, last, "c2f32_ab");
    else { make(1, first, first + 1, first + 2, -1, "c2f32_a"); make(2, -1, first + 3, first + 4, last, "c2f32_b"); }
    e->lazy_tensors.insert(e->tensors[cat].name);
    e->lazy_tensors.insert(e->tensors[tmp].name);
    return IRMV_OK;
}

// Single-frame steps: a 64-channel Bottleneck (model.6 / 12 / 18 at a 640 net) as ONE launch, the block's last one together
// with cv2 (k_bneck.hip).  The OP_BNECK ops stand behind the block's layer ops, which stay what batched steps run (and the
// bit-exactness reference); a step of one frame skips the layers and runs the fused launches instead.
static int fuse_bneck64(irmv_engine *e, const std::string &prefix, int n, bool shortcut, int cat, int out_t)
{
    if (!e->bneck64 || e->backbone != 0) return IRMV_OK;
    const int last = (int)e->ops.size() - 1, first = last - (2 * n + 1);
    if (n < 1 || n > 2 || first < 0) return IRMV_OK;
    for (int i = first; i <= last; i++)
        if (e->ops[i].kind != OP_CONV) return IRMV_OK;
    const Op &c2 = e->ops[last];
    bool ok = c2.cfg.ks == 1 && c2.cout == 128 && c2.cout_pad == 128 && c2.pair && c2.cin == (2 + n) * 64 && c2.ksteps == 2 * (2 + n) && c2.cfg.act == 1 &&
              !c2.cfg.out_f32 && c2.s1.C == 0 && c2.s0.shift == 0 && c2.res_t < 0;
    for (int i = first + 1; i < last && ok; i++) {
        const Op &m = e->ops[i];
        ok = m.cfg.ks == 3 && m.cfg.stride == 1 && m.cin == 64 && m.cout == 64 && m.pair && m.ksteps == 18 && m.cfg.act == 1 && !m.cfg.cin16 && m.w_lds[0] != nullptr &&
             m.s1.C == 0 && m.s0.shift == 0;
    }
    if (!ok) return IRMV_OK;
    const int bH = c2.Hin, bW = c2.Win;
    for (int i = 0; i < n; i++) {
        const int i_m1 = first + 1 + 2 * i, i_m2 = i_m1 + 1;
        const bool with_cv2 = i == n - 1;
        Op op;
        op.kind = OP_BNECK;
        op.mode = with_cv2 ? 1 : 0;
        op.shortcut = shortcut;
        op.layer = prefix + ".m." + std::to_string(i) + (with_cv2 ? " + cv2 (one launch)" : " (one launch)");
        snprintf(op.kname, sizeof op.kname, with_cv2 ? "bneck64_b" : "bneck64_a");
        op.sub[0] = i_m1; op.sub[1] = i_m2; op.sub[2] = with_cv2 ? last : -1;
        op.Hin = op.Hout = bH; op.Win = op.Wout = bW;
        op.out_t = with_cv2 ? out_t : cat;
        op.res_t = cat;
        const double px = (double)bH * bW;
        for (int k = 0; k < 3; k++)
            if (op.sub[k] >= 0) { op.flops += e->ops[op.sub[k]].flops; op.w_bytes += e->ops[op.sub[k]].w_bytes; }
        op.bytes = op.w_bytes + px * 64 * 2.0 + (with_cv2 ? px * (64.0 * n + 128.0) * 2.0 : px * 64 * 2.0);   // y_in once; + the other concat slices and the block output, or y_next
        op.bneck = 1;
        e->ops.push_back(op);
        const int me = (int)e->ops.size() - 1;
        e->ops[i_m1].bneck = me; e->ops[i_m2].bneck = me;
        if (with_cv2) e->ops[last].bneck = me;
    }
    e->lazy_tensors.insert(e->tensors[cat].name);   // (a single-frame step leaves the last slice of the concat buffer and the bottleneck intermediate unwritten:
    return IRMV_OK;                                 //  read-backs of them run the layer ops, like the fused 32-channel blocks')
}

// The keypoint branch of a Detect level -- the last three ops: 3x3 (Cin -> 16), 3x3 (16 -> 16) carrying the final 1x1 -- as one
// launch (k_kpt.hip).  The OP_KPT3 op stands behind the layer ops; a step runs it and skips them, read-backs of the two
// intermediate tensors run the layers (they remain the bit-exactness reference, IRMV_KPT3=0 the switch).
static int fuse_kpt3(irmv_engine *e, int level)
{
    if (!e->kpt3 || e->ops.size() < 3) return IRMV_OK;
    const int i2 = (int)e->ops.size() - 1, i1 = i2 - 1, i0 = i2 - 2;
    const Op &o0 = e->ops[i0], &o1 = e->ops[i1], &o2 = e->ops[i2];
    const bool ok = o0.kind == OP_CONV && o1.kind == OP_CONV && o2.kind == OP_CONV && o1.fuse_next == i2 && o1.cfg.cin16 && o2.w_k16 &&
                    o0.cfg.ks == 3 && o0.cfg.stride == 1 && o0.cfg.act == 1 && !o0.cfg.out_f32 && !o0.cfg.cin16 && o0.cout_pad == 16 && !o0.pair && o0.res_t < 0 &&
                    o0.s1.C == 0 && o0.s0.shift == 0 && o0.w_lds[0] != nullptr && kpt3_eligible(o0.cin) && o1.s0.t == o0.out_t && o1.cin == 16 && o1.ksteps == 5 &&
                    o0.Hin == o1.Hin && o0.Win == o1.Win;
    if (!ok) return IRMV_OK;
    {   // the kernel addresses the level's input through a buffer descriptor with 32-bit byte offsets
        const Tensor &xt = e->tensors[o0.s0.t];
        if ((double)e->cfg.num_slots * xt.H * xt.W * xt.C * 2.0 >= 2147483648.0) return IRMV_OK;
    }
    Op op;
    op.kind = OP_KPT3;
    op.layer = "model.22.cv4." + std::to_string(level) + " (one launch)";
    snprintf(op.kname, sizeof op.kname, "kpt3_c%d", o0.cin);
    op.sub[0] = i0; op.sub[1] = i1; op.sub[2] = i2;
    op.Hin = op.Hout = o0.Hin; op.Win = op.Wout = o0.Win;
    op.cin = o0.cin;
    op.level = level;
    op.flops = o0.flops + o1.flops + o2.flops;
    op.w_bytes = o0.w_bytes + o1.w_bytes + o2.w_bytes;
    op.out_bytes = o2.out_bytes;
    op.bytes = op.w_bytes + (o0.bytes - o0.w_bytes - o0.out_bytes) + o2.out_bytes;   // the level's input once, the head's keypoint channels once
    op.kpt3 = 1;
    e->lazy_tensors.insert(e->tensors[o0.out_t].name);
    e->lazy_tensors.insert(e->tensors[o1.out_t].name);
    e->ops.push_back(op);
    const int me = (int)e->ops.size() - 1;
    e->ops[i0].kpt3 = e->ops[i1].kpt3 = e->ops[i2].kpt3 = me;
    return IRMV_OK;
}

static int add_c2f(irmv_engine *e, const std::string &prefix, SegRef s0, SegRef s1, int H, int W, int c2, int n,
                   bool shortcut, int out_t)
{
    const int c = c2 / 2;
    int cat, tmp;
    TRY(new_tensor(e, prefix + ".cat", H, W, (2 + n) * c, false, &cat));
    TRY(new_tensor(e, prefix + ".tmp", H, W, c, false, &tmp));
    TRY(add_conv(e, prefix + ".cv1", s0, s1, H, W, cat, 0));
    for (int i = 0; i < n; i++) {
        const std::string m = prefix + ".m." + std::to_string(i);
        TRY(add_conv(e, m + ".cv1", SegRef{cat, (1 + i) * c, c, 0}, SegRef{}, H, W, tmp, 0));
        TRY(add_conv(e, m + ".cv2", SegRef{tmp, 0, c, 0}, SegRef{}, H, W, cat, (2 + i) * c, shortcut ? cat : -1,
                     (1 + i) * c));
    }
    TRY(add_conv(e, prefix + ".cv2", SegRef{cat, 0, (2 + n) * c, 0}, SegRef{}, H, W, out_t, 0));
    TRY(fuse_c2f32(e, prefix, n, shortcut, cat, tmp, out_t));
    if (c == 64) {
        TRY(fuse_bneck64(e, prefix, n, shortcut, cat, out_t));
        if (!e->ops.empty() && e->ops.back().kind == OP_BNECK) e->lazy_tensors.insert(e->tensors[tmp].name);
    }
    return IRMV_OK;
}

// integer tap geometry: same arithmetic as the oracle's axis_tap, written independently
static void axis_taps(std::vector<AxisTap> &out, int dn_total, int sn, int dn, int pad, bool rotate)
{
    out.assign(dn_total, AxisTap{-1, -1, 0, 0});
    for (int d = 0; d < dn_total; d++) {
        const int r = d - pad;
        if (r < 0 || r >= dn) continue;
        const long long num = (long long)(2 * r + 1) * sn - dn, den = 2LL * dn;
        const long long fl = num >= 0 ? num / den : -((-num + den - 1) / den);
        const long long frac = num - fl * den;
        int w = (int)((frac * 2048 + dn) / den);
        int a = (int)fl, b = a + 1;
        if (a < 0) { a = 0; b = 0; w = 0; }
        if (a >= sn - 1) { a = sn - 1; b = sn - 1; w = 0; }
        if (rotate) { a = sn - 1 - a; b = sn - 1 - b; }
        out[d] = AxisTap{a, b, w, 0};
    }
}

// The fused front kernel (k_front.hip) stages each tile's source region in LDS as 4-byte pixels, read in groups of
// 4 pixels = three aligned dwords: the width must be a multiple of 4 and the largest region must fit kFrontStageMax
// bytes of LDS.  Same box arithmetic as the kernel.
static int front_fits(const std::vector<AxisTap> &tx, const std::vector<AxisTap> &ty, int sw, int *tiles_x, int *tiles_y, int *stage_bytes,
                      int *pitch_out, int *rows_out)   // IRMV_FRONT_FUSED, or the reason it does not fit
{
    const int W1 = (int)tx.size() / 4, H1 = (int)ty.size() / 4;
    *tiles_x = (W1 + kFrontTileX - 1) / kFrontTileX;
    *tiles_y = (H1 + kFrontTileY - 1) / kFrontTileY;
    *stage_bytes = front_min_stage_bytes();
    *pitch_out = *rows_out = 0;
    if (sw % 4 != 0) return IRMV_FRONT_WIDTH_MOD4;   // 4-pixel groups = 12 source bytes read as three aligned dwords
    auto span = [&](const std::vector<AxisTap> &t, int g0, int n, int *lo, int *hi) {
        *lo = 0x7fffffff; *hi = -1;
        for (int i = g0; i < g0 + n; i++) {
            if (i < 0 || i >= (int)t.size() || t[i].i0 < 0) continue;
            *lo = std::min({*lo, t[i].i0, t[i].i1});
            *hi = std::max({*hi, t[i].i0, t[i].i1});
        }
    };
    int max_pitch = 0, max_rows = 0;
    for (int i = 0; i < *tiles_x; i++) {
        int lo, hi;
        span(tx, 4 * i * kFrontTileX - 3, 4 * kFrontTileX + 3, &lo, &hi);
        if (hi >= 0) max_pitch = std::max(max_pitch, std::min((hi + 4) & ~3, sw) - (lo & ~3));
    }
    for (int i = 0; i < *tiles_y; i++) {
        int lo, hi;
        span(ty, 4 * i * kFrontTileY - 3, 4 * kFrontTileY + 3, &lo, &hi);
        if (hi >= 0) max_rows = std::max(max_rows, hi - lo + 1);
    }
    *pitch_out = max_pitch; *rows_out = max_rows;
    if (max_pitch > 1023 || max_rows > 1023) return IRMV_FRONT_TAP_RANGE;   // region-relative taps are packed in 10 bits
    const size_t need = (size_t)max_pitch * max_rows * 4;
    *stage_bytes = std::max((int)std::min<size_t>((need + 255) & ~(size_t)255, 1u << 30), front_min_stage_bytes());
    return need <= (size_t)kFrontStageMax ? IRMV_FRONT_FUSED : IRMV_FRONT_STAGE_LIMIT;
}

// The upload kernel moves 16-byte words: the slots' first byte and their size must be multiples of 16.
static bool upload_aligned(size_t src_bytes, int first, int count)
{
    const size_t off = (size_t)first * src_bytes, bytes = src_bytes * count;
    return off % 16 == 0 && bytes % 16 == 0;
}

// Size of the resized frame inside the net input.  Letterbox into net_w x net_h: r = min(W / sw, H / sh), the scaled frame
// rounded (W == H: the square case); a stretch fills the net input.
static void scaled_size(const irmv_engine_cfg &c, int *nw, int *nh)
{
    const int net_w = c.net_size, net_h = c.net_height > 0 ? c.net_height : c.net_size;
    *nw = net_w; *nh = net_h;
    if (c.resize_mode != IRMV_RESIZE_LETTERBOX) return;
    const double r = std::min((double)net_w / c.src_width, (double)net_h / c.src_height);
    *nw = std::min(net_w, (int)std::floor(c.src_width * r + 0.5));
    *nh = std::min(net_h, (int)std::floor(c.src_height * r + 0.5));
}

// Every geometry decision of the network's front, from the configuration alone (no GPU): the letterbox box, the tap
// tables, whether the fused front kernel fits, its 2 : 1 column / direct / tall-tile path, and whether a single frame's
// upload can ride the upload kernel.  build_engine takes its geometry from here and irmv_front_plan exports it, so the
// exported plan is what runs.  `sw`: the engine's environment switches (IRMV_FRONT_FASTX / _DIRECT / _TILE8); all on
// for the exported plan.
struct FrontSwitches { bool fastx = true, direct = true, tall = true; };

static void front_plan(const irmv_engine_cfg &c, const FrontSwitches &sw, irmv_front_plan_t *p, std::vector<AxisTap> &tx, std::vector<AxisTap> &ty)
{
    const int net_w = c.net_size, net_h = c.net_height > 0 ? c.net_height : c.net_size;
    memset(p, 0, sizeof *p);
    // ---- preprocess geometry (parse_output inverse mapping): the scaled frame, centred ----
    int nw, nh;
    scaled_size(c, &nw, &nh);
    const int px = (net_w - nw) / 2, py = (net_h - nh) / 2;
    axis_taps(tx, net_w, c.src_width, nw, px, c.rotate180 != 0);
    axis_taps(ty, net_h, c.src_height, nh, py, c.rotate180 != 0);
    p->reason = front_fits(tx, ty, c.src_width, &p->tiles_x, &p->tiles_y, &p->stage_bytes, &p->max_pitch, &p->max_rows);
    p->fused = p->reason == IRMV_FRONT_FUSED;
    p->tile_y = kFrontTileY;
    p->box[0] = px; p->box[1] = px + nw; p->box[2] = py; p->box[3] = py + nh;
    {   // columns at exactly 2 : 1 (1280 -> 640): the taps of column px + k are the aligned source pair (m, m + 1) with
        // m = m0 + step k even, both weights 1/2; step = 2, or -2 under rotate180 (the pair is then listed as (m + 1, m):
        // with equal weights the blend does not care)
        const int step = c.rotate180 ? -2 : 2;
        const int m0 = nw > 0 ? std::min(tx[px].i0, tx[px].i1) : -1;
        bool fx = nw > 0 && m0 >= 0 && (m0 & 1) == 0;
        for (int d = px; d < px + nw && fx; d++)
            fx = std::min(tx[d].i0, tx[d].i1) == m0 + step * (d - px) && std::max(tx[d].i0, tx[d].i1) == m0 + step * (d - px) + 1 && tx[d].w1 == 1024;
        if (!sw.fastx) fx = false;
        const bool direct = fx && sw.direct;   // tiles without a padding pixel skip the LDS staging of the source (k_front.hip); bit 1 of FrontArgs::fastx
        p->fastx = fx ? (direct ? 3 : 1) : 0;
        // all tiles direct: nothing is staged, and the tile can be twice as tall (k_front.hip)
        if (fx && direct && p->fused && sw.tall) {
            p->tile_y = kFrontTileYDirect;
            p->tiles_y = (net_h / 4 + kFrontTileYDirect - 1) / kFrontTileYDirect;
            p->stage_bytes = front_min_stage_bytes(kFrontTileYDirect);
        }
        p->fx_i0 = fx ? m0 : 0;
        p->fx_step = step;
    }
    // the kernel's tile classes (k_front.hip tile_inside): a tile is inside on an axis when every net-input pixel it
    // reads on that axis, halo included, has a source
    const int inw = 4 * kFrontTileX + 3, inh = 4 * p->tile_y + 3;
    for (int j = 0; j < p->tiles_y; j++)
        for (int i = 0; i < p->tiles_x; i++) {
            const int gx0 = 4 * i * kFrontTileX - 3, gy0 = 4 * j * p->tile_y - 3;
            const bool in_x = gx0 >= std::max(p->box[0], 0) && gx0 + inw <= std::min(p->box[1], net_w);
            const bool in_y = gy0 >= std::max(p->box[2], 0) && gy0 + inh <= std::min(p->box[3], net_h);
            (in_x ? (in_y ? p->tiles_inside : p->tiles_y_edge) : (in_y ? p->tiles_x_edge : p->tiles_corner))++;
            if (j == 0 && (p->fastx & 2)) {   // the direct tiles' column pairing (k_front.hip mq, de, dg0): step sign x (mq & 3)
                const int mq = p->fx_i0 + p->fx_step * (gx0 - p->box[0]);
                p->pair_cases |= 1 << ((p->fx_step > 0 ? 0 : 2) + ((mq & 3) == 0 ? 0 : 1));
            }
        }
    // a single frame travels from its pinned slot as a kernel (upload_as_kernel) where the slot is aligned: slot 1 stands for all
    const size_t src_bytes = (size_t)c.src_width * c.src_height * (c.src_format != IRMV_SRC_HWC8 ? 1 : 3);
    p->upload_kernel = upload_aligned(src_bytes, 1, 1);
}

static int autotune_convs(irmv_engine *e);
static int write_window(irmv_engine *e, int slot);
static void finalize_head_fusion(irmv_engine *e);
static int build_head_groups(irmv_engine *e);
static void build_step_plans(irmv_engine *e);

// T[c][v] = lut[c][min(255, (v gain[c] + 128) >> 8)] from the engine's current gains and LUT -> isp_table_dev.  The caller has
// made sure that nothing of this engine is in flight.
static int write_isp_table(irmv_engine *e)
{
    uint8_t t[kBayerTableBytes];
    for (int c = 0; c < 3; c++)
        for (uint32_t v = 0; v < 256; v++) t[c * 256 + v] = e->isp_lut[c * 256 + std::min(255u, (v * e->isp_gain[c] + 128u) >> 8)];
    HIP_TRY(hipMemcpy(e->isp_table_dev, t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

// profile / op name of a Bayer engine's demosaic as it runs now
static const char *demosaic_kname(const irmv_engine *e) { return e->bayer_mhc ? "bayer_demosaic_mhc" : (e->bayer_table ? "bayer_demosaic_lut" : "bayer_demosaic"); }

static int build_engine(irmv_engine *e)
{
    const irmv_engine_cfg &c = e->cfg;
    const int net_w = c.net_size, net_h = c.net_height > 0 ? c.net_height : c.net_size, S = c.num_slots;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    // default: batched engines replay concurrent sub-batches of ~64 frames, two to four of them; a stream per slot
    // for engines of TripleBuffer size, whose single-slot steps then overlap
    e->num_streams = c.num_streams > 0 ? c.num_streams : (c.num_slots <= 4 ? c.num_slots : std::min(4, std::max(2, (c.num_slots + 127) / 128)));   // batched: two graphs of up to 128 frames (round 3: with the
                                                                                                                                                   // weights-resident / multi-block kernels larger graphs win: 256 frames as 2 x 128 +6 % over 192 as 3 x 64)
    { const char *bn = getenv("IRMV_BNECK64"); e->bneck64 = !(bn && bn[0] == '0'); }   // (read before the op list is built)
    { const char *kp = getenv("IRMV_KPT3"); e->kpt3 = !(kp && kp[0] == '0'); }
    if (const char *ns = getenv("IRMV_STREAMS")) e->num_streams = atoi(ns);
    e->num_streams = std::max(1, std::min({e->num_streams, 8, c.num_slots}));
    for (int i = 1; i < e->num_streams; i++) HIP_TRY(hipStreamCreateWithFlags(&e->extra_streams[i - 1], hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&e->h2d_stream, hipStreamNonBlocking));
    { const char *ic = getenv("IRMV_INLINE_COPIES"); e->inline_copies = ic && ic[0] == '1'; }
    { const char *gu = getenv("IRMV_GRAPH_UPLOAD"); e->graph_upload = !(gu && gu[0] == '0'); }
    e->slot_owner.assign(S, nullptr);
    e->frame_bytes = (size_t)c.src_width * c.src_height * 3;
    const bool bayer = c.src_format != IRMV_SRC_HWC8;
    e->full_bytes = (size_t)e->full_w * e->full_h * 3;   // (= frame_bytes without a window)
    e->src_bytes = bayer ? (size_t)e->full_w * e->full_h : e->full_bytes;
    {
        // NUMA-local frame slots (SURVEY section 7 "hard parts": on a full node the copy engines read 8 x 14 k FPS x 3.93 MB =
        // 440 GB/s of host memory): the creating thread runs on the CPUs of the GPU's own socket and prefers its memory while
        // the slots are allocated and first touched (hipHostMallocNumaUser = "follow the caller's policy"); affinity and
        // policy are restored afterwards.  IRMV_NUMA=0: plain hipHostMallocDefault wherever the thread happens to run.
        const char *nv = getenv("IRMV_NUMA");
        const bool want = e->numa_node >= 0 && !(nv && nv[0] == '0');
        numa::ScopedNode scope(want ? e->numa_node : -1);
        const bool user = want && scope.policy();
        HIP_TRY(hipHostMalloc((void **)&e->src_host, e->src_bytes * S, user ? (hipHostMallocDefault | hipHostMallocNumaUser) : hipHostMallocDefault));
        log_range(e, "pinned src_host", e->src_host, e->src_bytes * S);
        memset(e->src_host, 0, e->src_bytes * S);   // first touch, by the bound thread
        if (hipHostGetDevicePointer((void **)&e->src_host_dev, e->src_host, 0) != hipSuccess) { e->src_host_dev = nullptr; (void)hipGetLastError(); }
        if (const char *uk = getenv("IRMV_UPLOAD_KERNEL")) e->upload_kernel_blocks = atoi(uk);
        e->numa_placed = user && scope.bound();
    }
    TRY(dev_alloc(e, (void **)&e->src_dev, e->frame_bytes * S));
    HIP_TRY(hipMemset(e->src_dev, 0, e->frame_bytes * S));
    TRY(dev_alloc(e, (void **)&e->rot_dev, e->frame_bytes));
    if (e->window) {
        TRY(dev_alloc(e, (void **)&e->full_dev, e->full_bytes * S));
        HIP_TRY(hipMemset(e->full_dev, 0, e->full_bytes * S));
        TRY(dev_alloc(e, (void **)&e->win_dev, sizeof(int2) * S));
        { const char *wu = getenv("IRMV_WINDOW_UPLOAD"); e->window_upload = !(wu && wu[0] == '0'); }
    }
    if (bayer) {
        TRY(dev_alloc(e, (void **)&e->raw_dev, e->src_bytes * S));
        HIP_TRY(hipMemset(e->raw_dev, 0, e->src_bytes * S));
        // phase of the R sites: IRMV_SRC_BAYER_{RGGB, BGGR, GRBG, GBRG}8 -> R at (0,0), (1,1), (0,1), (1,0)
        static const int ry[4] = {0, 1, 0, 1}, rx[4] = {0, 1, 1, 0};
        BayerArgs &b = e->bayer;
        b.raw_slot_bytes = e->src_bytes; b.dst_slot_bytes = e->full_bytes;
        b.W = e->full_w; b.H = e->full_h;
        b.ry = ry[c.src_format - 1]; b.rx = rx[c.src_format - 1];
        for (int i = 0; i < 3; i++) b.gain[i] = c.bayer_gain_q8[i];
        for (int i = 0; i < 3; i++) e->isp_gain[i] = c.bayer_gain_q8[i];
        for (int i = 0; i < kBayerTableBytes; i++) e->isp_lut[i] = (uint8_t)(i & 255);
        TRY(dev_alloc(e, (void **)&e->isp_table_dev, kBayerTableBytes));
        e->bayer_mhc = c.bayer_demosaic == IRMV_DEMOSAIC_MHC;
        if (e->bayer_mhc) { e->bayer_table = true; TRY(write_isp_table(e)); }
    }

    // ---- preprocess and front geometry: front_plan, under this process's environment switches ----
    std::vector<AxisTap> tx, ty;
    irmv_front_plan_t plan;
    {
        FrontSwitches sw;
        if (const char *f = getenv("IRMV_FRONT_FASTX")) if (f[0] == '0') sw.fastx = false;
        if (const char *f = getenv("IRMV_FRONT_DIRECT")) if (f[0] == '0') sw.direct = false;
        if (const char *f = getenv("IRMV_FRONT_TILE8")) if (f[0] == '0') sw.tall = false;   // keeps the 4-row tile
        front_plan(c, sw, &plan, tx, ty);
    }
    const int px = plan.box[0], py = plan.box[2], nw = plan.box[1] - px, nh = plan.box[3] - py;
    TRY(dev_alloc(e, (void **)&e->tap_x, net_w * sizeof(AxisTap)));
    TRY(dev_alloc(e, (void **)&e->tap_y, net_h * sizeof(AxisTap)));
    HIP_TRY(hipMemcpy(e->tap_x, tx.data(), net_w * sizeof(AxisTap), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->tap_y, ty.data(), net_h * sizeof(AxisTap), hipMemcpyHostToDevice));
    e->fused_front = plan.fused != 0;
    e->front_tiles_x = plan.tiles_x; e->front_tiles_y = plan.tiles_y; e->front_stage_bytes = plan.stage_bytes;
    e->front_tile_y = plan.tile_y;
    for (int i = 0; i < 4; i++) e->front_v[i] = plan.box[i];
    e->front_fastx = plan.fastx; e->front_fx_i0 = plan.fx_i0; e->front_fx_step = plan.fx_step;
    if (const char *ff = getenv("IRMV_FUSED_FRONT")) if (ff[0] == '0') e->fused_front = false;
    if (e->fused_front && !front_prepare()) e->fused_front = false;

    // ---- graph ----
    // level sizes: h<s> x w<s> = net_h / s x net_w / s
    const int h2 = net_h / 2, h4 = net_h / 4, h8 = net_h / 8, h16 = net_h / 16, h32 = net_h / 32;
    const int w2 = net_w / 2, w4 = net_w / 4, w8 = net_w / 8, w16 = net_w / 16, w32 = net_w / 32;
    int x0, a0, a1, a2, a3, a4, a5, a6, a7, a8, s9, a9, a12, a15, a16, a18, a19, a21;
    TRY(new_tensor(e, "input", net_h, net_w, 4, false, &x0));
    TRY(new_tensor(e, "0", h2, w2, 16, false, &a0));
    TRY(new_tensor(e, "1", h4, w4, 32, false, &a1));
    const bool shuffle = e->backbone == 1;   // ShuffleNetV2 stages: blocks 2..8, P3 / P4 / P5 = tensors "3" / "6" / "8"
    if (shuffle) TRY(new_tensor(e, "2", h8, w8, 64, false, &a2));
    else TRY(new_tensor(e, "2", h4, w4, 32, false, &a2));
    TRY(new_tensor(e, "3", h8, w8, 64, false, &a3));
    if (shuffle) TRY(new_tensor(e, "4", h16, w16, 128, false, &a4));
    else TRY(new_tensor(e, "4", h8, w8, 64, false, &a4));
    TRY(new_tensor(e, "5", h16, w16, 128, false, &a5));
    TRY(new_tensor(e, "6", h16, w16, 128, false, &a6));
    TRY(new_tensor(e, "7", h32, w32, 256, false, &a7));
    TRY(new_tensor(e, "8", h32, w32, 256, false, &a8));
    TRY(new_tensor(e, "9.cat", h32, w32, 512, false, &s9));
    TRY(new_tensor(e, "9", h32, w32, 256, false, &a9));
    TRY(new_tensor(e, "12", h16, w16, 128, false, &a12));
    TRY(new_tensor(e, "15", h8, w8, 64, false, &a15));
    TRY(new_tensor(e, "16", h16, w16, 64, false, &a16));
    TRY(new_tensor(e, "18", h16, w16, 128, false, &a18));
    TRY(new_tensor(e, "19", h32, w32, 128, false, &a19));
    TRY(new_tensor(e, "21", h32, w32, 256, false, &a21));

    if (bayer) {   // raw slot -> src_dev: the first op of every step (not of run_post, not of a read-back's materialisation)
        Op op; op.kind = OP_DEMOSAIC; op.layer = "demosaic"; snprintf(op.kname, sizeof op.kname, "%s", demosaic_kname(e));
        op.bytes = (double)e->src_bytes + (double)e->full_bytes;
        e->ops.push_back(op);
    }
    if (e->window) {   // the slot's window -> src_dev: behind the demosaic, in front of everything else (like it, not part of run_post or a read-back)
        Op op; op.kind = OP_CROP; op.layer = "window_crop"; snprintf(op.kname, sizeof op.kname, "window_crop");
        op.bytes = 2.0 * (double)e->frame_bytes;
        e->ops.push_back(op);
    }
    const size_t conv0_op = e->ops.size() + 1;   // (OP_PRE, then OP_CONV0)
    { Op op; op.kind = OP_PRE; op.layer = "preprocess"; snprintf(op.kname, sizeof op.kname, "preprocess"); op.out_t = x0;
      op.bytes = (double)e->frame_bytes + (double)net_h * net_w * 8; e->ops.push_back(op); }
    {
        const LayerW *l = find_layer(e, "model.0.conv");
        if (!l || l->cin != 3 || l->cout != 16 || l->k != 3 || l->stride != 2)
            return fail(IRMV_ERR_MODEL, "model.0.conv missing or not 3x3 s2 3->16");
        // A fragments of the single 16-channel tile: lane (g, r) of k-step s holds channel r,
        // k = 32 s + 8 g + j  ->  kernel row kh = 2 s + (g >> 1), tap slot kw = 2 (g & 1) + (j >> 2), channel j & 3
        std::vector<uint16_t> w(2 * 64 * 8, 0);
        std::vector<float> b(16);
        for (int o = 0; o < 16; o++) b[o] = (float)((double)l->b[o] * (double)kActScale);   // (irmv_common.hpp, "activation scale")
        for (int ks = 0; ks < 2; ks++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int g = lane >> 4, o = lane & 15;
                    const int kh = 2 * ks + (g >> 1), kw = 2 * (g & 1) + (j >> 2), ci = j & 3;
                    if (kh < 3 && kw < 3 && ci < 3) w[((size_t)ks * 64 + lane) * 8 + j] = l->w[(o * 9 + kh * 3 + kw) * 3 + ci];
                }
        TRY(dev_alloc(e, (void **)&e->conv0_w, w.size() * 2));
        TRY(dev_alloc(e, (void **)&e->conv0_b, b.size() * 4));
        HIP_TRY(hipMemcpy(e->conv0_w, w.data(), w.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->conv0_b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
        Op op; op.kind = OP_CONV0; op.layer = "model.0.conv"; snprintf(op.kname, sizeof op.kname, "conv0_mfma");
        op.s0.t = x0; op.out_t = a0;
        op.flops = 2.0 * h2 * w2 * 16 * 27;
        op.bytes = (double)net_h * net_w * 8 + (double)h2 * w2 * 32 + 27 * 16 * 2;
        e->ops.push_back(op);
    }
    TRY(add_conv(e, "model.1.conv", SegRef{a0, 0, 16, 0}, SegRef{}, h2, w2, a1, 0));
    {
        const Op &m1 = e->ops.back();
        if (!(m1.cfg.cin16 && m1.ksteps == 5 && m1.pair && m1.cout_pad == 32 && m1.out_coff == 0)) e->fused_front = false;
        if (e->fused_front) {
            Op op; op.kind = OP_FRONT; op.layer = "preprocess+model.0+model.1"; snprintf(op.kname, sizeof op.kname, "front_fused");
            op.flops = e->ops[conv0_op].flops + m1.flops;
            op.bytes = (double)e->frame_bytes + (double)h4 * w4 * 32 * 2;
            op.w_packed = m1.w_packed; op.bias = m1.bias; op.out_t = m1.out_t;
            for (Op &o : e->ops) o.fused_away = o.kind != OP_DEMOSAIC && o.kind != OP_CROP;   // preprocess, model.0.conv, model.1.conv
            e->lazy_tensors.insert("input"); e->lazy_tensors.insert("0");
            e->ops.push_back(op);
        }
    }
    int p3 = a4, p4 = a6, p5 = a8;   // the tensors the neck reads
    if (shuffle) {
        TRY(add_shuffle_down(e, "model.2", a1, 32, h4, w4, 64, a2));
        TRY(add_shuffle_unit(e, "model.3", a2, 64, h8, w8, a3));
        TRY(add_shuffle_down(e, "model.4", a3, 64, h8, w8, 128, a4));
        TRY(add_shuffle_unit(e, "model.5", a4, 128, h16, w16, a5));
        TRY(add_shuffle_unit(e, "model.6", a5, 128, h16, w16, a6));
        TRY(add_shuffle_down(e, "model.7", a6, 128, h16, w16, 256, a7));
        TRY(add_shuffle_unit(e, "model.8", a7, 256, h32, w32, a8));
        p3 = a3;
    } else {
    TRY(add_c2f(e, "model.2", SegRef{a1, 0, 32, 0}, SegRef{}, h4, w4, 32, 1, true, a2));
    {
        // model.2 as one kernel (k_c2f.hip) when its four layers have the shapes that kernel is written for
        const int n = (int)e->ops.size();
        const Op &c1 = e->ops[n - 4], &m1 = e->ops[n - 3], &m2 = e->ops[n - 2], &c2 = e->ops[n - 1];
        bool ok = c1.cin == 32 && c1.cout == 32 && c1.cfg.ks == 1 && c1.pair && c1.ksteps == 1 &&
                  m1.cin == 16 && m1.cout == 16 && m1.cfg.cin16 && m1.ksteps == 5 && !m1.pair &&
                  m2.cin == 16 && m2.cout == 16 && m2.cfg.cin16 && m2.ksteps == 5 && !m2.pair && m2.res_t >= 0 &&
                  c2.cin == 48 && c2.cout == 32 && c2.cfg.ks == 1 && c2.pair && c2.ksteps == 2 &&
                  c1.cfg.act == 1 && m1.cfg.act == 1 && m2.cfg.act == 1 && c2.cfg.act == 1;
        if (const char *ff = getenv("IRMV_FUSED_C2F")) if (ff[0] == '0') ok = false;
        if (ok) {
            Op op; op.kind = OP_C2F2; op.layer = "model.2 (cv1+m.0+cv2)"; snprintf(op.kname, sizeof op.kname, "c2f2_fused");
            op.flops = c1.flops + m1.flops + m2.flops + c2.flops;
            op.bytes = 2.0 * (double)h4 * w4 * 32 * 2;
            for (int i = 0; i < 4; i++) { op.sub[i] = n - 4 + i; e->ops[n - 4 + i].fused_away = true; }
            op.s0 = c1.s0; op.out_t = c2.out_t;
            e->lazy_tensors.insert("model.2.cat"); e->lazy_tensors.insert("model.2.tmp");
            e->ops.push_back(op);
        }
    }
    TRY(add_conv(e, "model.3.conv", SegRef{a2, 0, 32, 0}, SegRef{}, h4, w4, a3, 0));
    TRY(add_c2f(e, "model.4", SegRef{a3, 0, 64, 0}, SegRef{}, h8, w8, 64, 2, true, a4));
    TRY(add_conv(e, "model.5.conv", SegRef{a4, 0, 64, 0}, SegRef{}, h8, w8, a5, 0));
    TRY(add_c2f(e, "model.6", SegRef{a5, 0, 128, 0}, SegRef{}, h16, w16, 128, 2, true, a6));
    TRY(add_conv(e, "model.7.conv", SegRef{a6, 0, 128, 0}, SegRef{}, h16, w16, a7, 0));
    TRY(add_c2f(e, "model.8", SegRef{a7, 0, 256, 0}, SegRef{}, h32, w32, 256, 1, true, a8));
    }
    TRY(add_conv(e, "model.9.cv1", SegRef{p5, 0, 256, 0}, SegRef{}, h32, w32, s9, 0));
    { Op op; op.kind = OP_POOL; op.layer = "model.9.m"; snprintf(op.kname, sizeof op.kname, "sppf_pool"); op.out_t = s9;
      op.bytes = (double)h32 * w32 * 128 * 2 * 4; e->ops.push_back(op); }
    TRY(add_conv(e, "model.9.cv2", SegRef{s9, 0, 512, 0}, SegRef{}, h32, w32, a9, 0));
    TRY(add_c2f(e, "model.12", SegRef{a9, 0, 256, 1}, SegRef{p4, 0, 128, 0}, h16, w16, 128, 1, false, a12));
    TRY(add_c2f(e, "model.15", SegRef{a12, 0, 128, 1}, SegRef{p3, 0, 64, 0}, h8, w8, 64, 1, false, a15));
    TRY(add_conv(e, "model.16.conv", SegRef{a15, 0, 64, 0}, SegRef{}, h8, w8, a16, 0));
    TRY(add_c2f(e, "model.18", SegRef{a16, 0, 64, 0}, SegRef{a12, 0, 128, 0}, h16, w16, 128, 1, false, a18));
    TRY(add_conv(e, "model.19.conv", SegRef{a18, 0, 128, 0}, SegRef{}, h16, w16, a19, 0));
    TRY(add_c2f(e, "model.21", SegRef{a19, 0, 128, 0}, SegRef{a9, 0, 256, 0}, h32, w32, 256, 1, false, a21));

    // Detect head: per level one fp32 record of kHeadRec per anchor: box 64 | cls 16 | kpt 16
    const int P[3] = {a15, a18, a21}, PC[3] = {64, 128, 256}, PH[3] = {h8, h16, h32}, PW[3] = {w8, w16, w32};
    int base = 0;
    for (int i = 0; i < 3; i++) {
        e->lvl_hw[i] = PH[i] * PW[i];
        e->lvl_base[i] = base;
        base += e->lvl_hw[i];
    }
    e->A = base;
    TRY(dev_alloc(e, (void **)&e->head_all, (size_t)S * e->A * kHeadRec * 4));
    HIP_TRY(hipMemset(e->head_all, 0, (size_t)S * e->A * kHeadRec * 4));
    for (int i = 0; i < 3; i++) {   // per-level views [slot][H*W][kHeadRec] into the one head allocation
        Tensor t;
        t.name = "head." + std::to_string(i);
        t.H = PH[i]; t.W = PW[i]; t.C = kHeadRec; t.f32 = true;
        t.slot_elems = (size_t)PH[i] * PW[i] * kHeadRec;
        t.base = e->head_all + (size_t)e->lvl_base[i] * S * kHeadRec;
        e->head_t[i] = (int)e->tensors.size();
        e->tensor_idx[t.name] = e->head_t[i];
        e->tensors.push_back(t);
    }
    const char *br[3] = {"cv2", "cv3", "cv4"};
    const int mid[3] = {64, 64, 16}, off[3] = {0, kClsOff, kKptOff};
    const int nbr = e->nk > 0 ? 3 : 2;
    // Engines that never batch (every step is a single frame: the reference node's shape) run the first-stage 3x3 convs of a
    // level's branches -- same input, 64 + 64 (+ 16) output channels -- as ONE conv: the weights are concatenated along
    // cout (keypoint branch padded to 32 channels with zeros), the second-stage convs read channel slices of the merged
    // output.  Same K order per output channel -> same bits; two or three launches fewer per level, and the level's input
    // is staged once.  Batched engines keep the separate convs (their nt = 4 tiles do not divide 160 channels).
    {
        const char *mh = getenv("IRMV_MERGE_HEAD0");
        e->merge_head0 = stream_share(e, S) == 1 && !(mh && mh[0] == '0');
        if (mh && mh[0] == '1') e->merge_head0 = true;
        for (int i = 0; i < 3 && e->merge_head0; i++)          // every branch conv must have the shape the merge assumes
            for (int b = 0; b < nbr; b++) {
                const LayerW *l0 = find_layer(e, std::string("model.22.") + br[b] + "." + std::to_string(i) + ".0");
                if (!l0 || l0->k != 3 || l0->stride != 1 || l0->act != 1 || l0->cin != PC[i] || l0->cout != mid[b]) e->merge_head0 = false;
            }
    }
    const int coff0[3] = {0, 64, 128};
    int t_s0[3] = {-1, -1, -1};
    if (e->merge_head0) {
        const int cm = nbr == 3 ? 160 : 128;
        e->merged_w.reserve(3); e->merged_b.reserve(3);
        e->layers.reserve(e->layers.size() + 3);      // LayerW pointers handed out below stay valid
        for (int i = 0; i < 3; i++) {
            const LayerW *src[3] = {nullptr, nullptr, nullptr};
            for (int b = 0; b < nbr; b++) src[b] = find_layer(e, std::string("model.22.") + br[b] + "." + std::to_string(i) + ".0");
            const size_t per_out = (size_t)9 * PC[i];
            e->merged_w.emplace_back((size_t)cm * per_out, (uint16_t)0);
            e->merged_b.emplace_back((size_t)cm, 0.f);
            for (int b = 0; b < nbr; b++) {
                memcpy(e->merged_w.back().data() + (size_t)coff0[b] * per_out, src[b]->w, (size_t)mid[b] * per_out * 2);
                memcpy(e->merged_b.back().data() + coff0[b], src[b]->b, (size_t)mid[b] * 4);
            }
            LayerW m;
            m.name = "model.22.s0." + std::to_string(i);
            m.cin = PC[i]; m.cout = cm; m.k = 3; m.stride = 1; m.act = 1;
            m.w = e->merged_w.back().data(); m.b = e->merged_b.back().data();
            e->layers.push_back(m);
            TRY(new_tensor(e, "22.s0." + std::to_string(i), PH[i], PW[i], cm, false, &t_s0[i]));
            TRY(add_conv(e, m.name, SegRef{P[i], 0, PC[i], 0}, SegRef{}, PH[i], PW[i], t_s0[i], 0));
            Op &mo = e->ops.back();
            const double real = nbr == 3 ? 144.0 : 128.0;
            mo.flops *= real / cm;                      // algorithmic work: the zero-padded channels do not count
            mo.level = i;
        }
    }
    for (int b = 0; b < nbr; b++)
        for (int i = 0; i < 3; i++) {
            const std::string pre = std::string("model.22.") + br[b] + "." + std::to_string(i);
            const std::string tn = std::string("22.") + br[b] + "." + std::to_string(i);
            int t1 = -1, t2;
            TRY(new_tensor(e, tn + ".1", PH[i], PW[i], mid[b], false, &t2));
            if (e->merge_head0) {
                TRY(add_conv(e, pre + ".1", SegRef{t_s0[i], coff0[b], mid[b], 0}, SegRef{}, PH[i], PW[i], t2, 0));
            } else {
                TRY(new_tensor(e, tn + ".0", PH[i], PW[i], mid[b], false, &t1));
                TRY(add_conv(e, pre + ".0", SegRef{P[i], 0, PC[i], 0}, SegRef{}, PH[i], PW[i], t1, 0));
                TRY(add_conv(e, pre + ".1", SegRef{t1, 0, mid[b], 0}, SegRef{}, PH[i], PW[i], t2, 0));
            }
            TRY(add_conv(e, pre + ".2", SegRef{t2, 0, mid[b], 0}, SegRef{}, PH[i], PW[i], e->head_t[i], off[b]));
            for (size_t k = e->ops.size() - (e->merge_head0 ? 2 : 3); k < e->ops.size(); k++) e->ops[k].level = i;
            {   // the branch's final 1x1 can ride in the epilogue of its second 3x3 (k_conv.hip, N2 > 0)
                const int i1 = (int)e->ops.size() - 2, i2 = i1 + 1;
                const Op &o1 = e->ops[i1], &o2 = e->ops[i2];
                const char *fh = getenv("IRMV_FUSED_HEAD");
                if (!(fh && fh[0] == '0') && o1.cout == 64 && o1.cin % 32 == 0 && o1.pair && o1.res_t < 0 && o1.cfg.stride == 1 &&
                    o2.cin == 64 && o2.ksteps == 2 && o2.cfg.ks == 1 && o2.cfg.out_f32 && o2.cfg.act == 0 && (o2.cout_pad == 16 || o2.cout_pad == 64))
                    e->ops[i1].fuse_next = i2;
                // ... and the keypoint branch's 16 -> nk final in the epilogue of the Cin = 16 direct kernel (one 16x16x16 MFMA per 16 pixels)
                if (!(fh && fh[0] == '0') && o1.cfg.cin16 && o1.cout_pad == 16 && !o1.pair && o1.res_t < 0 && o1.cfg.stride == 1 && o1.cfg.act == 1 && o2.w_k16)
                    e->ops[i1].fuse_next = i2;
            }
            if (b == 2 && !e->merge_head0) TRY(fuse_kpt3(e, i));
        }

    // ---- post-processing buffers ----
    TRY(dev_alloc(e, (void **)&e->boxes, (size_t)S * e->A * 16));
    TRY(dev_alloc(e, (void **)&e->keys, (size_t)S * e->A * e->nc * 8));
    // per-slot candidate counters of the split scan (k_post.hip scan_decode_kernel): zeroed HERE, once, with a synchronous
    // memset -- afterwards each nms_pnp launch reads its frames' counters and resets them itself (no memset node in a
    // captured step, nothing left non-zero between steps)
    { const char *sp = getenv("IRMV_SPLIT_SCAN"); e->split_scan = !(sp && sp[0] == '0'); }
    if (e->split_scan) {
        TRY(dev_alloc(e, (void **)&e->cand_counts, (size_t)S * sizeof(int)));
        HIP_TRY(hipMemset(e->cand_counts, 0, (size_t)S * sizeof(int)));
        // ... and the candidate-anchor bitmap of the sparse head, kept the same way
        e->cand_words = (e->A + 31) / 32;
        TRY(dev_alloc(e, (void **)&e->cand_bits, (size_t)S * e->cand_words * sizeof(unsigned int)));
        HIP_TRY(hipMemset(e->cand_bits, 0, (size_t)S * e->cand_words * sizeof(unsigned int)));
    }
    e->head_stale.assign((size_t)S, 0);
    e->branch_stale.assign((size_t)S, 0);
    TRY(dev_alloc(e, (void **)&e->dets_dev, (size_t)S * c.max_det * sizeof(DevDet)));
    TRY(dev_alloc(e, (void **)&e->fout_dev, (size_t)S * sizeof(DevFrameOut)));
    HIP_TRY(hipMemset(e->dets_dev, 0, (size_t)S * c.max_det * sizeof(DevDet)));
    HIP_TRY(hipMemset(e->fout_dev, 0, (size_t)S * sizeof(DevFrameOut)));
    // Result records live in mapped, coherent pinned memory: in keypoint mode the NMS kernel stores them there directly
    // (~20 KB per frame over PCIe, visible to the host once the stream is synchronised), which removes the D2H copies of
    // a step -- measured 9.6 us per synchronous call on this stack (scripts/probes/stream_probe.cpp), and copies issued
    // from the compute streams also halve the upload stream's H2D rate.  The classical mode (light_extract_kernel
    // reads and rewrites the records on the device) keeps device records + a copy.
    HIP_TRY(hipHostMalloc((void **)&e->dets_host, (size_t)S * c.max_det * sizeof(DevDet), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostMalloc((void **)&e->fout_host, (size_t)S * sizeof(DevFrameOut), hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void **)&e->dets_host_dev, e->dets_host, 0));
    HIP_TRY(hipHostGetDevicePointer((void **)&e->fout_host_dev, e->fout_host, 0));
    log_range(e, "pinned dets_host", e->dets_host, (size_t)S * c.max_det * sizeof(DevDet));
    log_range(e, "pinned fout_host", e->fout_host, (size_t)S * sizeof(DevFrameOut));
    memset(e->dets_host, 0, (size_t)S * c.max_det * sizeof(DevDet));
    memset(e->fout_host, 0, (size_t)S * sizeof(DevFrameOut));
    // class-logit scan + box decode of the candidate anchors: kScanBlocks workgroups per frame (k_post.hip)
    if (e->split_scan) {
        Op op; op.kind = OP_SCAN; op.layer = "scan_decode"; snprintf(op.kname, sizeof op.kname, "scan_decode");
        op.bytes = (double)e->A * 64.0; e->ops.push_back(op);
    }
    // [decode +] sort + NMS + keypoints + PnP: one kernel, one workgroup per frame (k_post.hip)
    { Op op; op.kind = OP_NMS; op.layer = "decode_nms_kpt_pnp"; snprintf(op.kname, sizeof op.kname, "nms_pnp");
      op.bytes = (double)e->A * 64.0; e->ops.push_back(op); }
    if (c.point_source == IRMV_POINTS_KEYPOINT_HEAD && e->nk < 8) return fail(IRMV_ERR_MODEL, "point_source = keypoint head, but the model has none");
    e->classical = c.point_source == IRMV_POINTS_CLASSICAL || (c.point_source == IRMV_POINTS_AUTO && e->nk < 8);
    { const char *z = getenv("IRMV_ZERO_COPY_RESULTS"); e->zero_copy_results = !e->classical && !(z && z[0] == '0'); }
    if (e->classical) {
        Op op; op.kind = OP_LIGHT; op.layer = "extract_armors"; snprintf(op.kname, sizeof op.kname, "light_extract");
        e->ops.push_back(op);
    }
    // scratch of the classical extraction: per detection a padded label image (ROIs up to ~510 x 510) and contour points
    const size_t SL = e->classical ? (size_t)S : 1;   // keypoint mode keeps one slot's worth for irmv_engine_extract_armors
    e->light_pool = std::max<size_t>((size_t)8 * c.src_width * c.src_height, (size_t)(c.src_width + 2) * (c.src_height + 2) + 16);
    TRY(dev_alloc(e, (void **)&e->light_labels, SL * e->light_pool));
    TRY(dev_alloc(e, (void **)&e->light_points, SL * c.max_det * kLightPointsCap * 2 * sizeof(short)));
    TRY(dev_alloc(e, (void **)&e->light_hulls, SL * c.max_det * kLightPointsCap * 4 * sizeof(short)));
    TRY(dev_alloc(e, (void **)&e->light_boxes, (size_t)c.max_det * 16));
    TRY(dev_alloc(e, (void **)&e->light_dets_dev, (size_t)c.max_det * sizeof(DevDet)));
    HIP_TRY(hipHostMalloc((void **)&e->light_dets_host, (size_t)c.max_det * sizeof(DevDet), hipHostMallocDefault));
    log_range(e, "pinned light_dets", e->light_dets_host, (size_t)c.max_det * sizeof(DevDet));

    PostArgs &p = e->post;
    p.net_w = net_w; p.net_h = net_h; p.A = e->A; p.nc = e->nc; p.nk = e->nk;
    p.logit_thr = (float)std::log((double)c.score_thr / (1.0 - (double)c.score_thr));
    p.iou_thr = c.iou_thr;
    p.max_det = c.max_det;
    p.pre_nms_cap = c.pre_nms_cap;
    { const char *pk = getenv("IRMV_POST_KEYS_ONLY"); e->post_keys_only = pk && pk[0] == '1'; }
    { const char *cw = getenv("IRMV_NMS_CLASSWALK"); p.classwalk = (cw && cw[0] == '0') ? 0 : 1; }
    { const char *pf = getenv("IRMV_NMS_PREFILTER"); p.prefilter = (pf && pf[0] == '0') ? 0 : 1;
      if (const char *pe = getenv("IRMV_NMS_PRE")) { int hi = 0, lo = 0; if (sscanf(pe, "%d,%d", &hi, &lo) == 2 && hi >= 64 && hi <= 512 && lo >= 32 && lo < hi) p.prefilter = hi | (lo << 16); } }   // experiment: size of the head of the list   // =0: crowded frames sort and mask every candidate (round-3 behaviour; bit-identical)
    if (c.resize_mode == IRMV_RESIZE_STRETCH) {
        p.scale_x = (float)c.src_width / (float)net_w;   // src/yolo_engine.cpp:155-156
        p.scale_y = (float)c.src_height / (float)net_h;
        p.off_x = p.off_y = 0.f;
    } else {
        p.scale_x = (float)c.src_width / (float)nw;
        p.scale_y = (float)c.src_height / (float)nh;
        p.off_x = (float)px;
        p.off_y = (float)py;
    }
    p.armor_size = c.armor_size;
    PnpConst pc;
    pc.fx = c.camera_matrix[0]; pc.fy = c.camera_matrix[4];
    pc.cx = c.camera_matrix[2]; pc.cy = c.camera_matrix[5];
    pc.k1 = c.dist_coeffs[0]; pc.k2 = c.dist_coeffs[1]; pc.p1 = c.dist_coeffs[2];
    pc.p2 = c.dist_coeffs[3]; pc.k3 = c.dist_coeffs[4];
    pc.hy[0] = 135.0 / 2.0 / 1000.0; pc.hy[1] = 225.0 / 2.0 / 1000.0;   // src/pnp_solver.cpp:18-21
    pc.hz[0] = pc.hz[1] = 55.0 / 2.0 / 1000.0;
    e->pnp_base = pc;
    TRY(dev_alloc(e, (void **)&e->pnp_dev, sizeof(PnpConst) * (e->window ? S : 1)));
    HIP_TRY(hipMemcpy(e->pnp_dev, &pc, sizeof pc, hipMemcpyHostToDevice));
    p.pnp = e->pnp_dev;
    p.pnp_stride = e->window ? 1 : 0;
    if (e->window) {   // every slot's window starts centred
        e->win_org.assign(S, int2{(e->full_w - c.src_width) / 2, (e->full_h - c.src_height) / 2});
        e->sub_org = e->win_org;
        for (int s = 0; s < S; s++) TRY(write_window(e, s));
    }
    p.dbg = nullptr;
    if (getenv("IRMV_NMS_STAMPS")) {
        TRY(dev_alloc(e, (void **)&e->dbg_dev, (size_t)S * 16 * sizeof(long long)));
        HIP_TRY(hipMemset(e->dbg_dev, 0, (size_t)S * 16 * sizeof(long long)));
        p.dbg = e->dbg_dev;
    }
    HIP_TRY(hipDeviceSynchronize());
    return IRMV_OK;
}

static int load_blob(irmv_engine *e)
{
    const irmv_engine_cfg &c = e->cfg;
    if (c.weights_path) {
        std::string path = c.weights_path;
        const size_t dot = path.find_last_of('.');
        if (dot != std::string::npos && path.substr(dot) != ".irmw") path = path.substr(0, dot) + ".irmw";
        std::ifstream f(path, std::ios::binary);
        if (!f) return fail(IRMV_ERR_MODEL, "cannot open weight blob " + path + " (convert the model to .irmw first)");
        f.seekg(0, std::ios::end);
        const size_t n = (size_t)f.tellg();
        f.seekg(0, std::ios::beg);
        e->blob.resize(n);
        f.read(reinterpret_cast<char *>(e->blob.data()), (std::streamsize)n);
    } else if (c.weights_blob && c.weights_bytes) {
        e->blob.resize(c.weights_bytes);
        if (c.weights_on_device) {
            HIP_TRY(hipSetDevice(c.device));
            HIP_TRY(hipMemcpy(e->blob.data(), c.weights_blob, c.weights_bytes, hipMemcpyDeviceToHost));
        } else {
            memcpy(e->blob.data(), c.weights_blob, c.weights_bytes);
        }
    } else {
        return fail(IRMV_ERR_MODEL, "no weights: set weights_path or weights_blob");
    }
    if (e->blob.size() < sizeof(BlobHeader)) return fail(IRMV_ERR_MODEL, "weight blob truncated");
    BlobHeader h;
    memcpy(&h, e->blob.data(), sizeof h);
    // dtype 1: fp16 weights.  dtype 2 (BASELINE configs[4], "int8 weights"): int8 OHWI weights + fp32 per-output-channel
    // scales; expanded here, once, to w = fp16(q * scale) -- the fragment packing below is dtype-agnostic from there on.
    if (memcmp(h.magic, "IRMW", 4) != 0 || h.version != 1 || (h.dtype != 1 && h.dtype != 2) || h.reg_max != 16)
        return fail(IRMV_ERR_MODEL, "not an IRMW v1 blob (fp16 or int8 weights)");
    e->dequant.reserve(h.n_layers);
    if (h.nc < 1 || h.nc > 16 || (h.nk != 0 && h.nk != 8))
        return fail(IRMV_ERR_MODEL, "unsupported head: nc must be 1..16, nk 0 or 8");
    if (h.reserved > 1) return fail(IRMV_ERR_MODEL, "unknown backbone id in the weight blob");
    e->backbone = (int)h.reserved;
    e->nc = (int)h.nc;
    e->nk = (int)h.nk;
    e->no = 64 + e->nc + e->nk;
    if (sizeof h + (size_t)h.n_layers * sizeof(BlobLayer) > e->blob.size()) return fail(IRMV_ERR_MODEL, "layer table truncated");
    for (uint32_t i = 0; i < h.n_layers; i++) {
        BlobLayer bl;
        memcpy(&bl, e->blob.data() + sizeof h + (size_t)i * sizeof bl, sizeof bl);
        LayerW l;
        char nm[33];
        memcpy(nm, bl.name, 32);
        nm[32] = 0;
        l.name = nm;
        l.cin = bl.cin; l.cout = bl.cout; l.k = bl.k; l.stride = bl.stride; l.act = bl.act;
        l.groups = bl.pad > 1 ? (int)bl.pad : 1;
        if (l.groups > 1 && !(l.groups == l.cout && l.cin == 1 && l.k == 3 && l.cout % 8 == 0 && l.act == 0))
            return fail(IRMV_ERR_MODEL, "layer " + l.name + ": only depthwise 3x3 grouped convs (no activation) are supported");
        const size_t nw = (size_t)l.cout * l.k * l.k * l.cin;
        const size_t w_bytes = h.dtype == 2 ? ((nw + 3) & ~(size_t)3) + (size_t)l.cout * 4 : nw * 2;
        if (bl.w_off + w_bytes > e->blob.size() || bl.b_off + (size_t)l.cout * 4 > e->blob.size())
            return fail(IRMV_ERR_MODEL, "layer " + l.name + " data out of range");
        l.w = reinterpret_cast<const uint16_t *>(e->blob.data() + bl.w_off);
        if (h.dtype == 2) {
            const int8_t *q = reinterpret_cast<const int8_t *>(e->blob.data() + bl.w_off);
            const float *scale = reinterpret_cast<const float *>(e->blob.data() + bl.w_off + ((nw + 3) & ~(size_t)3));
            e->dequant.emplace_back(nw);
            std::vector<uint16_t> &d = e->dequant.back();
            const size_t per_out = nw / l.cout;
            for (int o = 0; o < l.cout; o++)
                for (size_t i = 0; i < per_out; i++) d[o * per_out + i] = float_to_half_bits((float)q[o * per_out + i] * scale[o]);
            l.w = d.data();   // (the vectors were reserved above: no reallocation moves them)
        }
        l.b = reinterpret_cast<const float *>(e->blob.data() + bl.b_off);
        e->layers.push_back(l);
    }
    return IRMV_OK;
}

extern "C" void irmv_engine_cfg_default(irmv_engine_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0;
    cfg->src_width = 1280;
    cfg->src_height = 1024;
    cfg->net_size = 640;
    cfg->resize_mode = IRMV_RESIZE_STRETCH;
    cfg->rotate180 = 1;
    cfg->swap_rb = 0;
    cfg->score_thr = 0.25f;
    cfg->iou_thr = 0.45f;
    cfg->max_det = 100;
    cfg->pre_nms_cap = 4096;
    cfg->num_slots = 3;
    cfg->armor_size = IRMV_ARMOR_SMALL;
    // config/camera_info.yaml:7,12
    const double K[9] = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1};
    const double D[5] = {-0.405274, 0.126058, -0.026939, -0.006503, 0.0};
    memcpy(cfg->camera_matrix, K, sizeof K);
    memcpy(cfg->dist_coeffs, D, sizeof D);
    // src/irm_detector.cpp:152-173
    cfg->point_source = IRMV_POINTS_AUTO;
    cfg->binary_threshold = 150;
    cfg->light_min_ratio = 0.1f; cfg->light_max_ratio = 0.4f; cfg->light_max_angle = 40.0f;
    cfg->armor_min_small_center_distance = 0.8; cfg->armor_max_small_center_distance = 3.2;
    cfg->armor_min_large_center_distance = 3.2; cfg->armor_max_large_center_distance = 5.5;
    cfg->src_format = IRMV_SRC_HWC8;
    cfg->bayer_gain_q8[0] = cfg->bayer_gain_q8[1] = cfg->bayer_gain_q8[2] = 256;
}

// Which launch form serves detect() on this box: both timed on slot 0 (whatever its pinned slot holds: zeros at creation), the
// eager one kept only if it is at least 1 % faster.  IRMV_SYNC_LAUNCH=graph|eager skips the timing.
extern "C" int irmv_engine_submit(irmv_engine *e, int first, int count, uint32_t flags);
extern "C" int irmv_engine_wait_slots(irmv_engine *e, int first, int count);
static int choose_sync_launch(irmv_engine *e)
{
    if (const char *v = getenv("IRMV_SYNC_LAUNCH")) {
        if (v[0] == 'e' || v[0] == 'g') { e->sync_launch = v[0] == 'e' ? 1 : 0; return IRMV_OK; }   // (anything else, e.g. "auto": time it)
    }
    double t[2] = {0.0, 0.0};
    for (int round = 0; round < 2; round++)
        for (int mode = 0; mode < 2; mode++) {
            e->sync_launch = mode;
            for (int i = 0; i < 24; i++) {
                const auto t0 = std::chrono::high_resolution_clock::now();
                TRY(irmv_engine_submit(e, 0, 1, IRMV_SUBMIT_H2D));
                TRY(irmv_engine_wait_slots(e, 0, 1));
                if (i >= 8) t[mode] += std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count();
            }
        }
    e->sync_launch = t[1] < 0.99 * t[0] ? 1 : 0;
    if (getenv("IRMV_AUTOTUNE_VERBOSE")) fprintf(stderr, "[irmv] synchronous single-frame step: graph replay %.1f us, eager launches %.1f us -> %s\n", t[0] / 32, t[1] / 32, e->sync_launch ? "eager" : "graph");
    return IRMV_OK;
}

// struct_size of irmv_engine_cfg before src_format and the gains were appended
constexpr size_t kCfgSizeV1 = offsetof(irmv_engine_cfg, src_format);
// ... and before net_height: that header's sizeof.  net_height sits in its tail padding, so those bytes are never read.
constexpr size_t kCfgSizeV2 = offsetof(irmv_engine_cfg, reserved2);
static_assert(offsetof(irmv_engine_cfg, net_height) < kCfgSizeV2 && kCfgSizeV2 < sizeof(irmv_engine_cfg), "three distinct cfg sizes");
// The tracking window's two fields lie in what was the tail padding of the struct: its size is the one it had before them.
static_assert(offsetof(irmv_engine_cfg, win_width) == offsetof(irmv_engine_cfg, reserved2) + 4 && offsetof(irmv_engine_cfg, win_height) + 2 == sizeof(irmv_engine_cfg),
              "win_width / win_height fill the tail of irmv_engine_cfg");

// What everything behind the crop is built from: the configuration whose source frame is the window (itself without one).
static irmv_engine_cfg window_view(const irmv_engine_cfg &c)
{
    irmv_engine_cfg v = c;
    if (c.win_width > 0 && c.win_height > 0) { v.src_width = c.win_width; v.src_height = c.win_height; }
    v.win_width = v.win_height = 0;
    return v;
}

// The caller's configuration at this library's size (an older caller's prefix, the appended fields at their defaults),
// and the checks of everything the front's geometry follows from.  No GPU call.
static int resolve_cfg(const irmv_engine_cfg *cfg_in, irmv_engine_cfg *full)
{
    const size_t sz = cfg_in->struct_size;
    if (sz != sizeof(irmv_engine_cfg) && sz != kCfgSizeV1 && sz != kCfgSizeV2) return fail(IRMV_ERR_ARG, "irmv_engine_cfg size mismatch");
    if (sz != sizeof(irmv_engine_cfg)) {   // (the defaults include: no window)
        irmv_engine_cfg_default(full);
        memcpy(full, cfg_in, sz == kCfgSizeV1 ? kCfgSizeV1 : offsetof(irmv_engine_cfg, net_height));
        full->struct_size = sizeof *full;
        full->bayer_demosaic = IRMV_DEMOSAIC_BILINEAR;   // (the older headers had a reserved field there)
    } else {
        *full = *cfg_in;
    }
    const irmv_engine_cfg *cfg = full;
    if (cfg->src_format < IRMV_SRC_HWC8 || cfg->src_format > IRMV_SRC_BAYER_GBRG8) return fail(IRMV_ERR_ARG, "unknown src_format (IRMV_SRC_*)");
    if (cfg->bayer_demosaic > IRMV_DEMOSAIC_MHC) return fail(IRMV_ERR_ARG, "unknown bayer_demosaic (IRMV_DEMOSAIC_*)");
    if (cfg->bayer_demosaic == IRMV_DEMOSAIC_MHC) {
        if (cfg->src_format == IRMV_SRC_HWC8) return fail(IRMV_ERR_ARG, "bayer_demosaic = IRMV_DEMOSAIC_MHC needs a Bayer src_format (IRMV_SRC_BAYER_*8)");
        if (cfg->src_width < 4 || cfg->src_height < 4) return fail(IRMV_ERR_ARG, "bayer_demosaic = IRMV_DEMOSAIC_MHC needs src_width >= 4 and src_height >= 4 (reflect-101 at radius 2)");
    }
    if (cfg->src_format != IRMV_SRC_HWC8) {
        if (cfg->src_width % 2 || cfg->src_height % 2) return fail(IRMV_ERR_ARG, "a Bayer src_format (IRMV_SRC_BAYER_*8) needs an even src_width and src_height");
        for (int i = 0; i < 3; i++)
            if (cfg->bayer_gain_q8[i] > 1023) return fail(IRMV_ERR_ARG, "bayer_gain_q8 must be in [0, 1023] (Q8, 256 = 1.0)");
    }
    if (cfg->net_size < 64 || cfg->net_size % 32 != 0 || cfg->net_size > 2048) return fail(IRMV_ERR_ARG, "net_size must be a multiple of 32 in [64, 2048]");
    if (cfg->net_height != 0 && (cfg->net_height < 64 || cfg->net_height % 32 != 0 || cfg->net_height > 2048))
        return fail(IRMV_ERR_ARG, "net_height must be 0 (square) or a multiple of 32 in [64, 2048]");
    if (cfg->src_width < 2 || cfg->src_height < 2 || cfg->src_width > 4096) return fail(IRMV_ERR_ARG, "src size out of range (width <= 4096)");
    // The narrowest offset arithmetic of the kernels that read a source frame is the fused front's direct tiles (k_front.hip):
    // row * 3 src_width + 3 x + 11 as ONE unsigned 32-bit byte offset into the frame.  (preprocess_kernel, rotate180_kernel
    // and the light extraction index with size_t; the demosaic's int counts bytes of one band of rows.)
    if ((uint64_t)cfg->src_width * (uint64_t)cfg->src_height * 3u > IRMV_MAX_FRAME_BYTES)
        return fail(IRMV_ERR_ARG, "src frame too large: 3 * src_width * src_height must not exceed 4294967296 bytes (32-bit byte offsets into a frame)");
    // The tracking window: both 0 = none.  src_width x src_height stays the full frame (what the checks above bound); the
    // letterbox below, like everything behind the crop, sees the window.
    if (cfg->win_width < 0 || cfg->win_width > cfg->src_width) return fail(IRMV_ERR_ARG, "win_width must be 0 (no window) or in [1, src_width]");
    if (cfg->win_height < 0 || cfg->win_height > cfg->src_height) return fail(IRMV_ERR_ARG, "win_height must be 0 (no window) or in [1, src_height]");
    if ((cfg->win_width == 0) != (cfg->win_height == 0)) return fail(IRMV_ERR_ARG, "win_width and win_height must both be 0 (no window) or both be set");
    {   // a source so oblong that the short side of its letterboxed frame rounds to nothing: no box, no scale back to the source
        int nw, nh;
        scaled_size(window_view(*cfg), &nw, &nh);
        if (nw < 1 || nh < 1) return fail(IRMV_ERR_ARG, "letterbox: the scaled frame has no row or no column; use IRMV_RESIZE_STRETCH");
    }
    return IRMV_OK;
}

extern "C" int irmv_front_plan(const irmv_engine_cfg *cfg_in, irmv_front_plan_t *out)
{
    if (!cfg_in || !out) return fail(IRMV_ERR_ARG, "cfg/out is null");
    irmv_engine_cfg full;
    if (int rc = resolve_cfg(cfg_in, &full)) return rc;
    std::vector<AxisTap> tx, ty;
    front_plan(window_view(full), FrontSwitches{}, out, tx, ty);
    return IRMV_OK;
}

extern "C" int irmv_engine_create(const irmv_engine_cfg *cfg_in, irmv_engine **out)
{
    if (!cfg_in || !out) return fail(IRMV_ERR_ARG, "cfg/out is null");
    irmv_engine_cfg full;
    if (int rc = resolve_cfg(cfg_in, &full)) return rc;
    const irmv_engine_cfg *cfg = &full;
    if (cfg->num_slots < 1 || cfg->num_slots > 256) return fail(IRMV_ERR_ARG, "num_slots must be 1..256");
    if (cfg->max_det < 1 || cfg->max_det > IRMV_MAX_DET_CAP) return fail(IRMV_ERR_ARG, "max_det must be 1..256");
    if (cfg->pre_nms_cap < 1 || cfg->pre_nms_cap > IRMV_CAND_CAP) return fail(IRMV_ERR_ARG, "pre_nms_cap must be 1..8192");
    if (!(cfg->score_thr > 0.f && cfg->score_thr < 1.f)) return fail(IRMV_ERR_ARG, "score_thr must be in (0, 1)");
    if (cfg->armor_size != IRMV_ARMOR_SMALL && cfg->armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    if (cfg->point_source < 0 || cfg->point_source > 2) return fail(IRMV_ERR_ARG, "bad point_source");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(IRMV_ERR_HIP, "no such HIP device");
    std::unique_ptr<irmv_engine> e(new irmv_engine);
    e->cfg = window_view(*cfg);   // from here on: src_width x src_height = the window, where there is one
    e->window = cfg->win_width > 0;
    e->full_w = cfg->src_width; e->full_h = cfg->src_height;
    if (e->cfg.net_height == 0) e->cfg.net_height = e->cfg.net_size;   // from here on: net_size = width, net_height = height
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) e->num_cus = cus;
        int node = -1;
        if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, cfg->device) == hipSuccess) e->numa_node = node;
        else (void)hipGetLastError();   // an older runtime serving the library (torch's bundled ROCm 7.0) does not know the attribute: no node, and no sticky error for the checks behind the tuning launches
    }
    int rc = load_blob(e.get());
    e->cfg.weights_path = nullptr;  // caller-owned, not retained
    e->cfg.weights_blob = nullptr;
    if (rc) return rc;
    rc = build_engine(e.get());
    if (rc) return rc;
    rc = autotune_convs(e.get());
    if (rc) return rc;
    finalize_head_fusion(e.get());
    rc = build_head_groups(e.get());
    if (rc) return rc;
    build_step_plans(e.get());
    rc = choose_sync_launch(e.get());
    if (rc) return rc;
    *out = e.release();
    return IRMV_OK;
}

extern "C" int irmv_engine_sync_launch(const irmv_engine *e) { return e ? e->sync_launch : 0; }

extern "C" void irmv_engine_destroy(irmv_engine *e) { delete e; }
extern "C" int irmv_engine_num_slots(const irmv_engine *e) { return e ? e->cfg.num_slots : 0; }
extern "C" int irmv_engine_max_det(const irmv_engine *e) { return e ? e->cfg.max_det : 0; }
extern "C" int irmv_engine_num_streams(const irmv_engine *e) { return e ? e->num_streams : 0; }
extern "C" int irmv_engine_num_anchors(const irmv_engine *e) { return e ? e->A : 0; }
extern "C" int irmv_engine_net_dims(const irmv_engine *e, int *width, int *height)
{
    if (!e || !width || !height) return fail(IRMV_ERR_ARG, "engine/width/height is null");
    *width = e->cfg.net_size; *height = e->cfg.net_height;
    return IRMV_OK;
}
extern "C" int irmv_engine_numa_node(const irmv_engine *e) { return e ? e->numa_node : -1; }
extern "C" int irmv_engine_numa_placed(const irmv_engine *e) { return e && e->numa_placed ? 1 : 0; }

// ---- NUMA helpers for the threads / ranks that feed an engine (tools/irmv_multi_gpu.cpp, bench.py ranks) ----
extern "C" int irmv_numa_device_node(int device, int *node)
{
    if (!node) return fail(IRMV_ERR_ARG, "node is null");
    int v = -1;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeHostNumaId, device) != hipSuccess) {
        (void)hipGetLastError();        // (attribute unknown to the runtime that serves the library: not an error of the caller's)
        v = -1;
    }
    *node = v;
    return IRMV_OK;
}
extern "C" int irmv_numa_bind_thread(int node) { return numa::bind_thread_to_node(node) ? IRMV_OK : fail(IRMV_ERR_ARG, "no usable CPU on that NUMA node (or none listed in sysfs)"); }
extern "C" int irmv_numa_page_node(const void *p) { return numa::page_node(p); }
extern "C" int irmv_numa_parse_cpulist(const char *s, int *cpus, int cap)
{
    const std::vector<int> v = numa::parse_cpulist(s);
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) if (cpus) cpus[i] = v[i];
    return (int)v.size();
}
extern "C" int irmv_engine_head_channels(const irmv_engine *e) { return e ? e->no : 0; }

// the device memory an upload of the source slots writes: the raw slots of a Bayer engine, else the HWC frames themselves
// (a window engine's full frames)
static uint8_t *upload_dev(const irmv_engine *e) { return e->raw_dev ? e->raw_dev : (e->window ? e->full_dev : e->src_dev); }

extern "C" uint8_t *irmv_engine_src_buffer(irmv_engine *e, int slot)
{
    if (!e || slot < 0 || slot >= e->cfg.num_slots) return nullptr;
    return e->src_host + (size_t)slot * e->src_bytes;
}
extern "C" void *irmv_engine_src_device_buffer(irmv_engine *e, int slot)
{
    if (!e || slot < 0 || slot >= e->cfg.num_slots) return nullptr;
    return upload_dev(e) + (size_t)slot * e->src_bytes;
}
extern "C" int irmv_engine_src_format(const irmv_engine *e) { return e ? e->cfg.src_format : -1; }
extern "C" size_t irmv_engine_src_bytes(const irmv_engine *e) { return e ? e->src_bytes : 0; }

// ---- tracking window ----------------------------------------------------------------
// A window at (x0, y0) in result coordinates: where it lies in the buffer, the band of full-width rows it covers, and the
// principal point its pixels are seen with.  The one place this arithmetic lives (irmv_window_map exports it).
static int window_map(int full_w, int full_h, int win_w, int win_h, int rotate180, const double K[9], int x0, int y0, irmv_window_map_t *m)
{
    if (x0 < 0 || y0 < 0 || x0 > full_w - win_w || y0 > full_h - win_h) return fail(IRMV_ERR_ARG, "the window does not lie inside the frame");
    memset(m, 0, sizeof *m);
    m->bx0 = rotate180 ? full_w - x0 - win_w : x0;
    m->by0 = rotate180 ? full_h - y0 - win_h : y0;
    m->band_offset = (uint64_t)m->by0 * (uint64_t)full_w * 3u;
    m->band_bytes = (uint64_t)win_h * (uint64_t)full_w * 3u;
    m->cx = K[2] - (double)x0;
    m->cy = K[5] - (double)y0;
    return IRMV_OK;
}

extern "C" int irmv_window_map(const irmv_engine_cfg *cfg_in, int x0, int y0, irmv_window_map_t *out)
{
    if (!cfg_in || !out) return fail(IRMV_ERR_ARG, "cfg/out is null");
    irmv_engine_cfg full;
    if (int rc = resolve_cfg(cfg_in, &full)) return rc;
    if (full.win_width == 0) return fail(IRMV_ERR_ARG, "irmv_window_map: the configuration has no window (win_width, win_height)");
    return window_map(full.src_width, full.src_height, full.win_width, full.win_height, full.rotate180, full.camera_matrix, x0, y0, out);
}

// The slot's entries of the two device tables from e->win_org[slot].  The caller has made sure no step of the slot is in flight.
static int write_window(irmv_engine *e, int slot)
{
    irmv_window_map_t m;
    TRY(window_map(e->full_w, e->full_h, e->cfg.src_width, e->cfg.src_height, e->cfg.rotate180, e->cfg.camera_matrix, e->win_org[slot].x, e->win_org[slot].y, &m));
    const int2 b{m.bx0, m.by0};
    PnpConst pc = e->pnp_base;
    pc.cx = m.cx; pc.cy = m.cy;
    HIP_TRY(hipMemcpy(e->win_dev + slot, &b, sizeof b, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->pnp_dev + slot, &pc, sizeof pc, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_wait_slots(irmv_engine *e, int first, int count);
extern "C" int irmv_engine_set_window(irmv_engine *e, int slot, int x0, int y0)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->window) return fail(IRMV_ERR_ARG, "irmv_engine_set_window: the engine has no window (win_width, win_height)");
    if (slot < 0 || slot >= e->cfg.num_slots) return fail(IRMV_ERR_ARG, "slot out of range");
    irmv_window_map_t m;
    TRY(window_map(e->full_w, e->full_h, e->cfg.src_width, e->cfg.src_height, e->cfg.rotate180, e->cfg.camera_matrix, x0, y0, &m));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read both tables
    e->win_org[slot] = int2{x0, y0};
    return write_window(e, slot);
}

extern "C" int irmv_engine_get_window(const irmv_engine *e, int slot, int *x0, int *y0, int *w, int *h)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->window) return fail(IRMV_ERR_ARG, "irmv_engine_get_window: the engine has no window (win_width, win_height)");
    if (slot < 0 || slot >= e->cfg.num_slots) return fail(IRMV_ERR_ARG, "slot out of range");
    if (x0) *x0 = e->win_org[slot].x;
    if (y0) *y0 = e->win_org[slot].y;
    if (w) *w = e->cfg.src_width;
    if (h) *h = e->cfg.src_height;
    return IRMV_OK;
}

// tile choices already measured in this process, keyed by layer shape and batch (engines are created
// repeatedly in tests and by multi-slot nodes; the kernels and the device do not change in between)
// Process-wide and shared by every engine on every thread: all accesses hold g_tune_mu.
struct TuneEntry { int mt, nt, flags, ipw; };   // a choice as the IRMV_TUNE_CACHE file holds it (flags: tile_flags)
static bool operator==(const TuneEntry &x, const TuneEntry &y) { return x.mt == y.mt && x.nt == y.nt && x.flags == y.flags && x.ipw == y.ipw; }
static std::mutex g_tune_mu;
static std::map<std::string, TuneEntry> g_tune_cache;
static std::set<std::string> g_tune_files;   // IRMV_TUNE_CACHE paths already read

// A tile's family and options as one word (the cache file's third column): LDS family, deep prefetch, direct kernel in the
// LDS family's K order, pointwise kernel, two- / four-step staging, LDS family chunk-major over 2 / 4 images, 8-wave
// workgroup, resident weights (ipw = images per workgroup, any value), their ping-pong form
enum : int { T_LDS = 1, T_DEEP = 2, T_CT = 4, T_PW = 8, T_PF2 = 16, T_PF4 = 32, T_CM2 = 64, T_CM4 = 128, T_W8 = 256, T_WR = 512, T_PP = 1024 };
static int tile_flags(const ConvCfg &c)
{
    return (c.lds ? T_LDS : 0) | (c.deep ? T_DEEP : 0) | (c.ct ? T_CT : 0) | (c.pw ? T_PW : 0) | (c.pf2 ? T_PF2 : 0) | (c.pf4 ? T_PF4 : 0) |
           (c.cm == 2 ? T_CM2 : 0) | (c.cm == 4 ? T_CM4 : 0) | (c.w8 ? T_W8 : 0) | (c.wr ? T_WR : 0) | (c.pp ? T_PP : 0);
}
static TuneEntry tune_entry(const ConvCfg &c) { return {c.mt, c.nt, tile_flags(c), c.ipw}; }

// IRMV_TUNE_CACHE=<file>: persist the measured choices so that a profiled run (rocprofv3 --pmc ...)
// replays exactly the tiles of the benchmarked run without the tuning launches in its trace.  A path is read the first
// time an engine sees it; its entries replace the process's own for the same key.
static void tune_cache_load()
{
    const char *path = getenv("IRMV_TUNE_CACHE");
    if (!path) return;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (!g_tune_files.insert(path).second) return;
    std::ifstream f(path);
    std::string key;
    TuneEntry t;
    while (f >> key >> t.mt >> t.nt >> t.flags >> t.ipw) g_tune_cache[key] = t;
}

static void tune_cache_save()
{
    const char *path = getenv("IRMV_TUNE_CACHE");
    if (!path) return;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    std::ofstream f(path);
    for (auto &kv : g_tune_cache) f << kv.first << ' ' << kv.second.mt << ' ' << kv.second.nt << ' ' << kv.second.flags << ' ' << kv.second.ipw << '\n';
}

static ConvWeights conv_weights(const Op &op) { return {op.w_packed, {op.w_lds[0], op.w_lds[1], op.w_lds[2], op.w_lds[3]}, op.w_k16}; }

static bool run_conv(const Op &op, const ConvCfg &c, const ConvArgs &a, int count, hipStream_t s) { return launch_conv(c, a, conv_weights(op), count, s); }

// ---- per-layer tile autotuner ---------------------------------------------------
// Every conv layer is timed at its real shape with each (MT, NT) tile the kernel
// family offers and keeps the fastest, once for full batched steps and once for
// single-frame steps.  All tiles walk K in the same order, so the choice never
// changes a single output bit (tests/test_gpu_engine.py::test_tile_choice_is_bitwise_neutral).
static void fill_conv_args(const irmv_engine *e, const Op &op, int first, int count, ConvArgs &a, bool fused = false);

// A candidate of the autotuner: the layer's own configuration with a tile shape, family and options (tile_flags' word).
static ConvCfg tile_cfg(const ConvCfg &base, int mt, int nt, int flags, int ipw)
{
    ConvCfg c = base;
    c.mt = mt; c.nt = nt; c.ipw = ipw;
    c.lds = flags & T_LDS; c.deep = flags & T_DEEP; c.ct = flags & T_CT; c.pw = flags & T_PW; c.pf2 = flags & T_PF2; c.pf4 = flags & T_PF4;
    c.cm = (flags & T_CM2) ? 2 : ((flags & T_CM4) ? 4 : 0); c.w8 = flags & T_W8; c.wr = flags & T_WR; c.pp = flags & T_PP;
    return c;
}

static TuneSwitches tune_switches()
{
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    const char *at = getenv("IRMV_AUTOTUNE"), *nd = getenv("IRMV_NO_DEEP");
    TuneSwitches s;
    s.untuned = at && at[0] == '0'; s.verbose = on("IRMV_AUTOTUNE_VERBOSE"); s.warn = on("IRMV_TUNE_WARN");
    const char *s2 = getenv("IRMV_FORCE_S2"), *wres = getenv("IRMV_FORCE_WRES");
    s.has_s2 = s2 != nullptr; s.force_s2 = s2 ? s2 : "";
    s.has_wres = wres != nullptr; s.force_wres = wres ? wres : "";
    s.force_pw = on("IRMV_FORCE_PW"); s.force_pwn = on("IRMV_FORCE_PWN"); s.force_cm = on("IRMV_FORCE_CM");
    s.force_w8 = on("IRMV_FORCE_W8"); s.force_nt8 = on("IRMV_FORCE_NT8"); s.force_pf4 = on("IRMV_FORCE_PF4");
    s.no_pw = on("IRMV_NO_PW"); s.no_pwn = on("IRMV_NO_PWN"); s.no_pf2 = on("IRMV_NO_PF2"); s.no_pf4 = on("IRMV_NO_PF4");
    s.no_cm = on("IRMV_NO_CM"); s.no_w8 = on("IRMV_NO_W8"); s.no_nt8 = on("IRMV_NO_NT8"); s.no_wres = on("IRMV_NO_WRES");
    s.no_deep = nd && nd[0] == '1';
    return s;
}

// forced: an IRMV_FORCE_* switch puts the layer on this candidate (parity tests) -- the last forced one that runs is the choice
struct TuneCand { ConvCfg c; bool forced; };

// Every candidate of one conv layer at one batch, in the order the tuner times them (IRMV_AUTOTUNE=0 takes the first that
// runs; a cached choice is replayed only if it is one of them).  Launches nothing: a candidate is listed if resolve_conv
// finds a kernel for it on this layer, the one that run_conv launches.  lds_ok: the layer's kernel family; want_fuse: the
// fused 1x1 epilogue, which needs an LDS-family tile that owns all 64 channels (nt = 4).
static std::vector<TuneCand> tune_candidates(const Op &op, const ConvArgs &a, int count, bool want_fuse, bool lds_ok, const TuneSwitches &sw, int num_cus)
{
    std::vector<TuneCand> v;
    // IRMV_FORCE_S2=lds|ct|deep (parity test): the stride-2 layers of the LDS family on ONE of their three bit-identical
    // implementations -- the LDS kernel, the direct kernel walking K chunk-major, its deep-prefetch form
    const bool s2 = sw.has_s2 && lds_ok && op.cfg.stride == 2;
    const ConvWeights w = conv_weights(op);
    auto add = [&](const ConvCfg &c, bool forced = false) {
        if (s2 && !forced && sw.force_s2 != (c.lds ? "lds" : (c.deep ? "deep" : "ct"))) return;
        if (resolve_conv(c, a, w, count)) v.push_back({c, forced});
    };
    const int ipw_max = lds_ok ? std::min(4, count) : 1;
    for (int mt = 1; mt <= 4; mt *= 2)
        for (int nt = 1; nt <= 4; nt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
                if (!want_fuse || nt == 4) add(tile_cfg(op.cfg, mt, nt, lds_ok ? T_LDS : 0, ipw));
    // LDS family, smallest pixel tile, staging two steps ahead (layers whose step is shorter than a memory round trip)
    if (lds_ok && !want_fuse && !sw.no_pf2)
        for (int nt = 1; nt <= 4; nt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2) add(tile_cfg(op.cfg, 1, nt, T_LDS | T_PF2, ipw));
    // ... and four steps ahead: layers of four or more chunks on maps small enough for four register sets (a lone frame's
    // 20 x 20 layers: every step of a workgroup in flight at once)
    if (lds_ok && !want_fuse && !sw.no_pf4 && op.cin >= 128) add(tile_cfg(op.cfg, 1, 1, T_LDS | T_PF4, 1), sw.force_pf4);
    // LDS family, chunk-major over the workgroup's images: a chunk's weights staged once for all of them
    if (lds_ok && !sw.no_cm)
        for (int mt = 1; mt <= 2; mt *= 2)
            for (int ipw = 2; ipw <= std::min(mt == 1 ? 4 : 2, count); ipw *= 2)
                add(tile_cfg(op.cfg, mt, 4, T_LDS | (ipw == 2 ? T_CM2 : T_CM4), ipw), sw.force_cm);
    // LDS family, stride 2: one 8-wave workgroup per CU on a block twice as tall (mt = 2 fits LDS, weights staged for
    // twice the pixels)
    if (lds_ok && op.cfg.stride == 2 && !want_fuse && !sw.no_w8)
        for (int mt = 1; mt <= 2; mt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
                for (int cmv = 0; cmv < 2; cmv++)
                    add(tile_cfg(op.cfg, mt, 4, T_LDS | T_W8 | (cmv ? (ipw == 2 ? T_CM2 : T_CM4) : 0), ipw), sw.force_w8);
    // ... and with all of 128 output channels per workgroup (nt = 8, mt = 1): these layers are bound by what a CU can stage
    // from L2 (12 B/clk), and the stride-2 patch -- four input pixels per output pixel -- is then fetched once per 128
    // channels instead of once per 64; chunk-major over two images halves the weight staging on top
    if (lds_ok && op.cfg.stride == 2 && !want_fuse && !sw.no_w8 && !sw.no_nt8)
        for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
            for (int cmv = 0; cmv < 2; cmv++)
                add(tile_cfg(op.cfg, 1, 8, T_LDS | T_W8 | (cmv ? T_CM2 : 0), ipw), sw.force_nt8);
    // LDS family, Cin = Cout = 64, stride 1: resident weights (one 8-wave workgroup per CU walks ipw images at its tile
    // position; lockstep, or as two ping-pong groups of four waves).  ipw: the smallest that lets the chip hold the
    // grid in one round, and half of it.
    if (lds_ok && count >= 2 && !sw.no_wres)
        for (int ppv = 0; ppv < 2; ppv++) {
            const int wgt = conv_wres_tiles(a, op.cfg.stride, ppv != 0);
            if (wgt <= 0) continue;
            int ipw1 = 1;
            while (ipw1 < count && (long)wgt * ((count + ipw1 - 1) / ipw1) > num_cus) ipw1++;
            const int cand[3] = {ipw1, (ipw1 + 1) / 2, std::min(count, 2 * ipw1)};
            for (int k = 0; k < 3; k++)
                if (k == 0 || (cand[k] != cand[0] && (k == 1 || cand[2] != cand[1]))) add(tile_cfg(op.cfg, 2, 4, T_LDS | T_WR | (ppv ? T_PP : 0), cand[k]));
        }
    // parity tests: IRMV_FORCE_WRES=<n> puts every eligible layer on the resident-weights kernel with n images per
    // workgroup -- the ping-pong form (listed last, so it wins) where the map tiles into its blocks (n < 0: never), else the
    // lockstep form
    if (sw.has_wres && lds_ok && count >= 2) {
        const int n = atoi(sw.force_wres.c_str());
        for (int ppv = 0; ppv <= (n > 0 ? 1 : 0); ppv++) add(tile_cfg(op.cfg, 2, 4, T_LDS | T_WR | (ppv ? T_PP : 0), std::max(1, std::min(count, n < 0 ? -n : n))), true);
    }
    // 1x1 layers: the persistent pointwise kernel (same operands, same k order as the direct kernel)
    if (conv_pw_eligible(op.cfg, a) && !sw.no_pw) {
        add(tile_cfg(op.cfg, 2, 4, T_PW, 1), sw.force_pw);
        // ... and its multi-block form: one workgroup runs a pixel tile against 2 / 4 output-channel blocks (input read once)
        for (int nbw = 2; nbw <= 4 && !sw.no_pwn; nbw *= 2)
            add(tile_cfg(op.cfg, 2, 4, T_PW, nbw), sw.force_pwn);   // (forced: the widest form offered)
    }
    // A layer of the LDS family may also run on the direct kernel walking K in that family's order on its weights (ct):
    // bit-identical, so the family rule still holds.  Offered where the direct kernel has a chance: stride 2.
    if (lds_ok && !want_fuse && op.cfg.stride == 2 && !op.cfg.cin16)
        for (int mt = 1; mt <= 4; mt *= 2)
            for (int nt = 1; nt <= 4; nt *= 2) add(tile_cfg(op.cfg, mt, nt, T_CT, 1));
    // single-frame steps: the latency variants of the direct kernel (deep prefetch ring), same rule.
    // Batched steps: offered to the 1x1 layers only (4..16 k-steps: the ring then holds the wave's whole K range).
    if ((count == 1 || op.cfg.ks == 1) && !want_fuse && !sw.no_deep && !op.cfg.cin16 && !op.cfg.out_f32 && op.cfg.act == 1) {
        const int tiles[4][2] = {{1, 1}, {2, 1}, {1, 2}, {1, 4}};
        for (auto &t : tiles) add(tile_cfg(op.cfg, t[0], t[1], T_DEEP | (lds_ok ? T_CT : 0), 1));
    }
    return v;
}

// How the tuner sees a conv op on slots [first, first + count): its arguments, whether it is tuned for its branch's final
// 1x1 in the epilogue (op.fuse_next), and its kernel family.  autotune_convs and the conv test hooks both use it.
struct ConvView { ConvArgs a; bool want_fuse, lds_ok; };
static ConvView conv_view(const irmv_engine *e, const Op &op, int first, int count)
{
    ConvView v;
    const ConvWeights w = conv_weights(op);
    const bool fuse_k16 = op.fuse_next >= 0 && op.cfg.cin16;   // the keypoint final in the direct kernel's epilogue: any pixel tile (nt = 1 is the layer's only one)
    v.want_fuse = op.fuse_next >= 0 && !fuse_k16;
    fill_conv_args(e, op, first, count, v.a, v.want_fuse || fuse_k16);
    if (v.want_fuse) {   // the fused epilogue needs an LDS-family tile that owns all 64 channels (nt = 4)
        bool f_ok = false;
        for (int mt = 1; mt <= 4 && !f_ok; mt *= 2) f_ok = conv_lds_fits(v.a, w, op.cfg.stride, mt, 4);
        if (!f_ok) {
            v.want_fuse = false;
            fill_conv_args(e, op, first, count, v.a, false);
        }
    }
    // Kernel family by a rule that does not depend on the batch (the two families walk K in
    // different orders): LDS-staged whenever some tile of it fits this layer, else direct.
    v.lds_ok = false;
    if (op.cfg.ks == 3 && op.cfg.act == 1 && !op.cfg.out_f32)
        for (int mt = 1; mt <= 4 && !v.lds_ok; mt *= 2)
            for (int nt = 1; nt <= 4 && !v.lds_ok; nt *= 2) v.lds_ok = conv_lds_fits(v.a, w, op.cfg.stride, mt, nt);
    return v;
}

static int autotune_convs(irmv_engine *e)
{
    const TuneSwitches sw = tune_switches();
    e->tune_sw = sw;
    tune_cache_load();
    hipEvent_t ea, eb;
    HIP_TRY(hipEventCreate(&ea));
    HIP_TRY(hipEventCreate(&eb));
    const int counts[2] = {stream_share(e, e->cfg.num_slots), 1};   // the batch one graph actually runs; single frame
    for (Op &op : e->ops) {
        if (op.kind != OP_CONV) continue;
        for (int pass = 0; pass < (counts[0] > 1 ? 2 : 1); pass++) {
            const int count = counts[pass];
            op.tune_fuse[pass] = op.fuse_next;
            const ConvView v = conv_view(e, op, 0, count);
            if (!v.want_fuse && !op.cfg.cin16) op.fuse_next = -1;   // no tile can carry the 1x1: the layers stay apart
            const ConvArgs &a = v.a;
            const bool want_fuse = v.want_fuse, lds_ok = v.lds_ok;
            char key[160];
            snprintf(key, sizeof key, "gfx950.t5|%d.%d.%d.%d.%d.%d|%dx%d>%dx%d|c%d.%d.%d.%d>%d|ld%d.%d.%d|n%d|%d", op.cfg.ks, op.cfg.stride,   // ".t5": the table format / flag set of round 5 -- entries of another round's file never match, so they are re-tuned, not reinterpreted
                     (int)op.cfg.cin16, op.cfg.act, (int)op.cfg.out_f32, (int)lds_ok, a.Hin, a.Win, a.Hout, a.Wout, a.s0.C, a.s1.C, a.s0.shift,
                     a.s1.shift, a.cout_pad, a.s0.ld, a.s1.ld, a.out_ld, count, (a.res ? 1 : 0) + 2 * a.n2);
            const std::vector<TuneCand> cands = tune_candidates(op, a, count, want_fuse, lds_ok, sw, e->num_cus);
            // a forced layer neither replays a cached choice nor leaves its own for a later engine; nor does an untuned one
            const bool forced = (sw.has_s2 && lds_ok && op.cfg.stride == 2) || std::any_of(cands.begin(), cands.end(), [](const TuneCand &k) { return k.forced; });
            ConvCfg best_cfg = pass == 0 ? op.cfg : op.cfg_one;
            bool have_hit = false;
            if (!forced && !sw.untuned && !sw.verbose) {   // a cached choice (this process, or an IRMV_TUNE_CACHE file) is replayed if it is a candidate
                std::lock_guard<std::mutex> lk(g_tune_mu);
                auto hit = g_tune_cache.find(key);
                if (hit != g_tune_cache.end()) {
                    const TuneEntry &h = hit->second;
                    auto it = std::find_if(cands.begin(), cands.end(), [&](const TuneCand &k) { return tune_entry(k.c) == h; });
                    if (it != cands.end()) { best_cfg = it->c; have_hit = true; }
                    else if (sw.warn) fprintf(stderr, "[autotune] cached tile for %s rejected (mt %d nt %d lds %d ipw %d): re-tuning\n", key, h.mt, h.nt, h.flags & 1, h.ipw);
                }
            }
            float best = 1e30f;
            for (size_t i = 0; i < cands.size() && !have_hit; i++) {
                const ConvCfg &c = cands[i].c;
                if (cands[i].forced) {
                    if (run_conv(op, c, a, count, e->stream)) { best = 0.f; best_cfg = c; }
                    continue;
                }
                if (sw.untuned && best < 1e29f) continue;   // IRMV_AUTOTUNE=0: the first candidate that runs is the choice
                bool ok = true;
                for (int r = 0; r < 2 && ok; r++) ok = run_conv(op, c, a, count, e->stream);
                if (!ok) continue;
                if (sw.untuned) { best = 0.f; best_cfg = c; continue; }
                float ms = 1e30f;   // best of 3 bursts of 4
                for (int rep = 0; rep < 3; rep++) {
                    HIP_TRY(hipEventRecord(ea, e->stream));
                    for (int r = 0; r < 4; r++) run_conv(op, c, a, count, e->stream);
                    HIP_TRY(hipEventRecord(eb, e->stream));
                    HIP_TRY(hipEventSynchronize(eb));
                    float t = 0.f;
                    HIP_TRY(hipEventElapsedTime(&t, ea, eb));
                    ms = t < ms ? t : ms;
                }
                if (sw.verbose) {
                    char nm[48];
                    conv_cfg_name(c, nm, sizeof nm);
                    fprintf(stderr, "[autotune] %-22s count=%-2d %-28s %8.2f us\n", op.layer.c_str(), count, nm, ms / 4 * 1e3);
                }
                if (ms < best) { best = ms; best_cfg = c; }
            }
            if (!forced && !sw.untuned) { std::lock_guard<std::mutex> lk(g_tune_mu); g_tune_cache[key] = tune_entry(best_cfg); }
            if (pass == 0) { op.cfg = best_cfg; conv_cfg_name(op.cfg, op.kname, sizeof op.kname); }
            else { op.cfg_one = best_cfg; conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one); }
            if (counts[0] == 1) { op.cfg_one = op.cfg; conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one); }
        }
    }
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    HIP_TRY(hipGetLastError());
    tune_cache_save();
    return IRMV_OK;
}

// a class-branch conv that carries its final 1x1: with emit_scan, its epilogue appends the level's scan candidates
static bool is_cls_final_carrier(const Op &op) { return op.fuse_next >= 0 && op.level >= 0 && op.layer.rfind("model.22.cv3.", 0) == 0; }

// A 3x3 conv carries its branch's final 1x1 only if BOTH of its tile choices can (LDS family, nt = 4); then the 1x1
// op drops out of the step and the tensor between the two is no longer written.
static void finalize_head_fusion(irmv_engine *e)
{
    for (Op &op : e->ops) {
        if (op.fuse_next < 0) continue;
        const bool k16 = op.cfg.cin16 && !op.cfg.lds && !op.cfg_one.lds && !op.cfg.deep && !op.cfg_one.deep && op.cfg.nt == 1 && op.cfg_one.nt == 1 && e->ops[op.fuse_next].w_k16;
        const bool ok = k16 || (op.cfg.lds && op.cfg.nt == 4 && op.cfg_one.lds && op.cfg_one.nt == 4);
        if (!ok) { op.fuse_next = -1; continue; }
        e->ops[op.fuse_next].fused_away = true;
        e->lazy_tensors.insert(e->tensors[op.out_t].name);
        const size_t l = strlen(op.kname), l1 = strlen(op.kname_one);
        snprintf(op.kname + l, sizeof op.kname - l, "+1x1");
        snprintf(op.kname_one + l1, sizeof op.kname_one - l1, "+1x1");
    }
    // candidate emission from the conv epilogues: only if the class branch of EVERY level ends in a fused 1x1
    int fused = 0;
    for (const Op &op : e->ops) fused += is_cls_final_carrier(op);
    const char *ev = getenv("IRMV_EMIT_SCAN");
    e->emit_scan = e->split_scan && fused == 3 && !(ev && ev[0] == '0');
    const char *sh = getenv("IRMV_SPARSE_HEAD");
    e->sparse_head = e->emit_scan && e->cand_bits && !(sh && sh[0] == '0');
    const char *sb = getenv("IRMV_SPARSE_BRANCH");
    e->sparse_branch = e->sparse_head && !(sb && sb[0] == '0');
}

// ---- grouped Detect-branch launches (single-frame engines) ---------------------------
static void scan_args_for(const irmv_engine *e, const Op &op, const PostArgs &pa, ConvArgs &a)
{
    a.scan_keys = pa.keys; a.scan_counts = pa.counts; a.scan_thr = pa.logit_thr; a.scan_nc = pa.nc;
    a.scan_key_cap = pa.key_cap;
    a.scan_abase = e->lvl_base[op.level];
    a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words;   // (sparse head: the class channels stay on chip)
}

// one launch for all members of group g on slot `first`; member k appends candidates to pa's key lists if bit k of `scan` is set
static bool launch_head_group(const irmv_engine *e, const irmv_engine::HeadGroup &g, int first, const PostArgs *pa, unsigned scan, hipStream_t s)
{
    ConvArgs a[kMultiMax];
    ConvWeights w[kMultiMax];
    const int n = (int)g.members.size();
    for (int k = 0; k < n; k++) {
        const Op &op = e->ops[g.members[k]];
        fill_conv_args(e, op, first, 1, a[k], true);
        if (scan >> k & 1u) scan_args_for(e, op, *pa, a[k]);
        w[k] = conv_weights(op);
    }
    return g.family == 0 ? launch_conv_lds_multi(g.nt, a, w, n, 1, s) : launch_conv_direct_multi(g.cfg, a, n, s);
}

static int build_head_groups(irmv_engine *e)
{
    const char *gh = getenv("IRMV_GROUP_HEAD");
    if (!e->merge_head0 || (gh && gh[0] == '0')) return IRMV_OK;
    auto find_op = [&](const std::string &layer) {
        for (size_t i = 0; i < e->ops.size(); i++)
            if (e->ops[i].kind == OP_CONV && !e->ops[i].fused_away && e->ops[i].layer == layer) return (int)i;
        return -1;
    };
    auto time_of = [&](auto &&launch) {   // ms per launch, or < 0 if it cannot run
        for (int i = 0; i < 2; i++) if (!launch()) return -1.f;
        if (hipStreamSynchronize(e->stream) != hipSuccess) return -1.f;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1.f;
        (void)hipEventRecord(a, e->stream);
        for (int i = 0; i < 8; i++) launch();
        (void)hipEventRecord(b, e->stream);
        (void)hipEventSynchronize(b);
        float ms = -1.f;
        (void)hipEventElapsedTime(&ms, a, b);
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        return ms / 8.f;
    };
    auto members_time = [&](const std::vector<int> &mem) {
        return time_of([&] {
            for (int i : mem) {
                const Op &op = e->ops[i];
                ConvArgs a;
                fill_conv_args(e, op, 0, 1, a, true);
                if (!run_conv(op, op.cfg_one, a, 1, e->stream)) return false;
            }
            return true;
        });
    };
    auto try_group = [&](std::vector<int> mem, int family, std::vector<int> nts, const char *label) {
        for (int i : mem) if (i < 0) return;
        if (mem.size() < 2 || mem.size() > (size_t)kMultiMax) return;
        irmv_engine::HeadGroup best;
        float best_ms = -1.f;
        for (int nt : nts) {
            irmv_engine::HeadGroup g;
            g.members = mem; g.family = family; g.nt = nt;
            if (family == 1) {
                g.cfg = e->ops[mem[0]].cfg_one;
                bool same = !g.cfg.lds && !g.cfg.ct && !g.cfg.pw;   // (the members' own tile shapes and prefetch depths are bitwise neutral: the group runs mt = nt = 1)
                for (int i : mem) {
                    const ConvCfg &c = e->ops[i].cfg_one;
                    same = same && c.ks == g.cfg.ks && c.stride == g.cfg.stride && c.cin16 == g.cfg.cin16 && c.act == g.cfg.act && c.out_f32 == g.cfg.out_f32 && !c.lds && !c.ct && !c.pw;
                }
                if (!same) continue;
                g.cfg.mt = g.cfg.nt = 1; g.cfg.deep = false;
            } else {
                bool fam = true;   // every member must belong to the LDS family's K order (its single-frame choice is an LDS tile or the CT stand-in)
                for (int i : mem) fam = fam && (e->ops[i].cfg_one.lds || e->ops[i].cfg_one.ct);
                if (!fam) continue;
            }
            if (getenv("IRMV_GROUP_VERBOSE")) { fprintf(stderr, "[irmv group] timing %s nt %d ...\n", label, nt); fflush(stderr); }
            const float ms = time_of([&] { return launch_head_group(e, g, 0, nullptr, 0u, e->stream); });
            if (getenv("IRMV_GROUP_VERBOSE")) { fprintf(stderr, "[irmv group] ... %.2f us\n", ms * 1e3f); fflush(stderr); }
            if (ms > 0.f && (best_ms < 0.f || ms < best_ms)) { best_ms = ms; best = g; }
        }
        if (best_ms < 0.f) return;
        const float sep = members_time(mem);
        if (getenv("IRMV_AUTOTUNE_VERBOSE") || getenv("IRMV_GROUP_VERBOSE")) fprintf(stderr, "[irmv group] %s: %zu convs, one launch %.2f us, separate %.2f us\n", label, mem.size(), best_ms * 1e3f, sep * 1e3f);
        if (sep > 0.f && best_ms >= sep && !getenv("IRMV_GROUP_FORCE")) return;   // IRMV_GROUP_FORCE=1 (parity test): group even where the one launch timed slower
        if (family == 0) snprintf(best.name, sizeof best.name, "%s_lds_mt1_nt%d_x%zu", label, best.nt, mem.size());
        else snprintf(best.name, sizeof best.name, "%s_direct_x%zu", label, mem.size());
        const int gi = (int)e->head_groups.size();
        e->head_groups.push_back(best);
        for (int i : mem) e->ops[i].group = gi;
    };
    const bool kpt = e->nk > 0;
    std::vector<int> g1, g2, g3, g4;
    bool g2_fused = true;
    for (int i = 0; i < 3; i++) {
        const std::string si = std::to_string(i);
        g1.push_back(find_op("model.22.s0." + si));
        const int c2 = find_op("model.22.cv2." + si + ".1"), c3 = find_op("model.22.cv3." + si + ".1");
        g2.push_back(c2); g2.push_back(c3);
        g2_fused = g2_fused && c2 >= 0 && c3 >= 0 && e->ops[c2].fuse_next >= 0 && e->ops[c3].fuse_next >= 0;
        if (kpt) { g3.push_back(find_op("model.22.cv4." + si + ".1")); g4.push_back(find_op("model.22.cv4." + si + ".2")); }
    }
    try_group(g1, 0, {1, 2}, "head_s0");
    if (g2_fused) try_group(g2, 0, {4}, "head_s1+1x1");
    // A group is launched where its FIRST member stands in the op list, so every member's input must exist by then.  The
    // first-stage convs precede all of these; the keypoint finals (cv4.i.2) read cv4.i.1, and cv4.1.1 / cv4.2.1 stand BEHIND
    // cv4.0.2 in the list: the finals may only be grouped when the convs before them are (one launch, at cv4.0.1's place).
    if (kpt) {
        const size_t before = e->head_groups.size();
        try_group(g3, 1, {1}, "head_kpt1");
        bool k16 = false;   // (finals on the 16x16x16 MFMA are fused into the convs in front of them, or run their own kernel: the grouped direct kernel would give other bits)
        for (int i : g4) k16 = k16 || i < 0 || e->ops[i].w_k16 != nullptr;
        if (e->head_groups.size() > before && !k16) try_group(g4, 1, {1}, "head_kpt2");
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// ---- step plans ------------------------------------------------------------------
// a box-branch conv that carries its final 1x1 (the 64 DFL channels of the head rows)
static bool is_box_final_carrier(const Op &op) { return op.fuse_next >= 0 && op.level >= 0 && op.layer.rfind("model.22.cv2.", 0) == 0; }

// Sparse head: the launches that write head rows store only those of candidate anchors, so within a step every class carrier
// (it finds the candidates) has to run in front of them.  A step is a linear chain; the op list has the box branches first.
// The box carriers move behind the last class carrier -- they read their own branch's first conv only and nothing in between
// reads the head, so no bit changes -- and then they and the keypoint launches are marked.  Launches this does not reach
// keep every row: a grouped launch (single-frame engines: box and class finals of all levels in ONE launch, no order to
// be had) and the keypoint branch as layers.  The head bytes of a marked launch, and of every emitting class carrier, no longer
// count as written: what is left is 96 floats per candidate anchor.
//
// Sparse branch (e->sparse_branch): the marked launches also carry the tile gate -- a (tile, image) pair without a candidate
// anchor stores nothing, so the resident-weight kernels and the keypoint kernel do not compute it (halo 0).  The box branch's
// first conv feeds nothing but its carrier's 3x3: where it runs a resident-weight kernel it moves behind the last class carrier
// too (it reads the level input only) and is gated with a halo of one pixel; its tensor becomes a lazy one (Op::gated_first).
// flops / bytes stay the dense figures: upper bounds for a gated launch.
static void sparse_head_plan(irmv_engine *e, std::vector<Launch> &plan)
{
    int last_cls = -1;
    bool lvl_cls[3] = {false, false, false};
    for (size_t i = 0; i < plan.size(); i++)
        if (plan[i].scan && plan[i].group < 0) { last_cls = (int)i; lvl_cls[e->ops[plan[i].op].level] = true; }
    auto box_carrier = [&](const Launch &l) {
        const Op &op = e->ops[l.op];
        return l.group < 0 && l.fused && op.kind == OP_CONV && is_box_final_carrier(op) && op.level < 3 && lvl_cls[op.level];
    };
    std::vector<char> first_conv(plan.size(), 0);   // resident-weight launches whose output tensor is read by a box carrier of this plan and by no other op
    if (e->sparse_branch)
        for (size_t i = 0; i < plan.size(); i++) {
            const Launch &f = plan[i];
            const Op &fo = e->ops[f.op];
            if (f.group >= 0 || f.fused || f.scan || fo.kind != OP_CONV || !(f.cfg_one ? fo.cfg_one : fo.cfg).wr || fo.res_t >= 0) continue;
            int carrier = -1;
            for (size_t j = i + 1; j < plan.size(); j++) {
                const Op &co = e->ops[plan[j].op];
                if (box_carrier(plan[j]) && co.level == fo.level && co.s0.t == fo.out_t && co.s1.C == 0 && co.s0.coff == fo.out_coff && co.Hin == fo.Hout && co.Win == fo.Wout) carrier = plan[j].op;
            }
            bool other = false;   // any other reader of the tensor (or a second writer) would see it stale outside active tiles
            for (int k = 0; k < (int)e->ops.size(); k++) {
                const Op &o = e->ops[k];
                if (k == carrier || k == f.op) continue;
                other = other || o.s0.t == fo.out_t || o.s1.t == fo.out_t || o.res_t == fo.out_t || o.out_t == fo.out_t;
            }
            first_conv[i] = carrier >= 0 && !other;
        }
    std::vector<Launch> out, moved;
    for (size_t i = 0; i < plan.size(); i++) {
        Launch &l = plan[i];
        Op &op = e->ops[l.op];
        if (l.scan) {   // class carrier(s): the 1x1's output stays on chip
            if (l.group < 0) l.bytes -= e->ops[op.fuse_next].out_bytes;
            else for (size_t m = 0; m < e->head_groups[l.group].members.size(); m++)
                if (l.scan >> m & 1u) l.bytes -= e->ops[e->ops[e->head_groups[l.group].members[m]].fuse_next].out_bytes;
        }
        const bool cls_first = op.level >= 0 && op.level < 3 && lvl_cls[op.level];
        const bool box = box_carrier(l);
        const bool kpt = op.kind == OP_KPT3 && cls_first && (int)i > last_cls;
        if (box || kpt) {
            l.sparse = true;
            l.bytes -= box ? e->ops[op.fuse_next].out_bytes : op.out_bytes;
            if (e->sparse_branch) l.gate = 1;
        }
        if (first_conv[i]) {
            l.gate = 2;
            op.gated_first = true;
            e->lazy_tensors.insert(e->tensors[op.out_t].name);
        }
        if ((box || first_conv[i]) && (int)i < last_cls) moved.push_back(l); else out.push_back(l);
        if ((int)i == last_cls) { out.insert(out.end(), moved.begin(), moved.end()); moved.clear(); }
    }
    plan.swap(out);
}

// The one place that decides which ops of e->ops a step of each kind launches, and how.
static void build_step_plans(irmv_engine *e)
{
    for (int k = STEP_BATCH; k <= STEP_POST; k++) {
        const bool one = k == STEP_ONE, mat = k == STEP_MATERIALIZE, post = k == STEP_POST, step = !mat && !post;
        auto emits = [&](const Op &op) { return step && e->emit_scan && is_cls_final_carrier(op); };
        for (int i = 0; i < (int)e->ops.size(); i++) {
            const Op &op = e->ops[i];
            if (post && op.kind != OP_NMS && op.kind != OP_LIGHT && op.kind != OP_SCAN) continue;
            if (op.kind == OP_SCAN && e->emit_scan && !post) continue;   // the class-branch convs have already filled the key lists
            const bool grouped = one && op.kind == OP_CONV && op.group >= 0;
            if (grouped && e->head_groups[op.group].members[0] != i) continue;   // rides in its group's launch
            // single-frame steps: the 64-channel Bottlenecks ride in their OP_BNECK launch; every other kind runs the layers
            const bool bneck = one && e->bneck64;
            if (op.kind == OP_BNECK ? !bneck : (op.bneck >= 0 && bneck)) continue;
            // every step runs a level's keypoint branch as its OP_KPT3 launch (where the engine has one)
            if (op.kind == OP_KPT3 ? !step : (op.kpt3 >= 0 && step)) continue;
            // a step skips the layers a fused kernel covers; a read-back runs only those (and the unfused form of a conv that
            // normally carries a 1x1 in its epilogue)
            // (... and a box branch's first conv that the steps -- their plans are built first -- run behind the tile gate)
            if (mat ? !(op.fused_away || op.fuse_next >= 0 || op.gated_first || ((op.bneck >= 0 || op.kpt3 >= 0) && op.kind == OP_CONV)) : op.fused_away) continue;
            Launch l; l.op = i;
            // every kernel is idempotent and can be repeated inside its profile bracket -- except the light extraction and, with
            // the split scan, the scan / NMS pair (the scan appends to the frame's candidate list, the NMS kernel consumes and resets it)
            l.once = op.kind == OP_LIGHT || (e->split_scan && (op.kind == OP_SCAN || op.kind == OP_NMS));
            l.keys_only = op.kind == OP_NMS && ((e->emit_scan && !post) || (post && e->post_keys_only));
            l.layer = op.layer;
            if (grouped) {   // one launch for the whole group
                const irmv_engine::HeadGroup &g = e->head_groups[op.group];
                l.group = op.group;
                l.name = g.name;
                l.layer += " ... (" + std::to_string(g.members.size()) + " convs)";
                for (size_t m = 0; m < g.members.size(); m++) {
                    const Op &mo = e->ops[g.members[m]];
                    if (emits(mo)) l.scan |= 1u << m;
                    l.flops += mo.flops + (mo.fuse_next >= 0 ? e->ops[mo.fuse_next].flops : 0.0);
                    l.bytes += mo.bytes;
                }
            } else {
                l.cfg_one = op.kind == OP_CONV && (one || mat) && stream_share(e, e->cfg.num_slots) > 1;   // (a read-back runs one slot)
                l.fused = !mat && op.fuse_next >= 0;
                l.scan = emits(op) ? 1u : 0u;
                l.name = l.cfg_one ? op.kname_one : op.kname;
                const Op *nx = l.fused ? &e->ops[op.fuse_next] : nullptr;   // the fused 1x1's output is what reaches memory, its weights ride along
                l.flops = op.flops + (nx ? nx->flops : 0.0);
                l.launch_bytes = op.w_bytes + (nx ? nx->w_bytes : 0.0);
                l.bytes = op.bytes + (nx ? nx->out_bytes - op.out_bytes + nx->w_bytes : 0.0) - l.launch_bytes;
            }
            e->plans[k].push_back(l);
        }
        if (step && e->sparse_head) sparse_head_plan(e, e->plans[k]);
    }
}

// ---- step execution ------------------------------------------------------------
struct EvRec { hipEvent_t a = nullptr, b = nullptr; };
constexpr int kProfileRepeat = 4;   // launches per event bracket in irmv_engine_profile

static void fill_conv_args(const irmv_engine *e, const Op &op, int first, int count, ConvArgs &a, bool fused)
{
    a = ConvArgs{};
    auto seg = [&](const SegRef &s) {
        ConvSeg cs{nullptr, 0, 0, 0};
        if (s.t < 0 || s.C == 0) return cs;
        const Tensor &t = e->tensors[s.t];
        cs.p = static_cast<const half_t *>(t.slot(first)) + s.coff;
        cs.ld = t.C;
        cs.C = s.C;
        cs.shift = s.shift;
        return cs;
    };
    a.s0 = seg(op.s0);
    a.s1 = seg(op.s1);
    a.Hin = op.Hin; a.Win = op.Win; a.Hout = op.Hout; a.Wout = op.Wout;
    a.M = count * op.Hout * op.Wout;
    a.Cin = op.cin;
    a.w = op.w_packed;
    a.bias = op.bias;
    const Tensor &ot = e->tensors[op.out_t];
    a.out = static_cast<char *>(ot.slot(first)) + (size_t)op.out_coff * ot.esize();
    a.out_ld = ot.C;
    a.res = nullptr;
    a.res_ld = 0;
    if (op.res_t >= 0) {
        const Tensor &rt = e->tensors[op.res_t];
        a.res = static_cast<const half_t *>(rt.slot(first)) + op.res_coff;
        a.res_ld = rt.C;
    }
    a.cout_pad = op.cout_pad;
    a.ksteps = op.ksteps;
    a.pair = op.pair ? 1 : 0;
    a.w2 = nullptr; a.bias2 = nullptr; a.out2 = nullptr; a.out2_ld = 0; a.n2 = 0;
    if (fused && op.fuse_next >= 0) {
        const Op &o2 = e->ops[op.fuse_next];
        const Tensor &t2 = e->tensors[o2.out_t];
        a.w2 = op.cfg.cin16 ? o2.w_k16 : o2.w_packed;
        a.bias2 = o2.bias;
        a.out2 = static_cast<float *>(t2.slot(first)) + o2.out_coff;
        a.out2_ld = t2.C;
        a.n2 = o2.cout_pad / 16;
    }
    if (op.w_k16) a.w2 = op.w_k16;   // a Cin = 16 final as its own launch (k_conv.hip conv1x1_k16_f32_kernel)
}

static LightArgs light_args(const irmv_engine *e, int first)
{
    LightArgs a{};
    const irmv_engine_cfg &c = e->cfg;
    a.frames = e->src_dev + (size_t)first * e->frame_bytes;
    a.frame_bytes = e->frame_bytes;
    a.cols = c.src_width; a.rows = c.src_height; a.rotate180 = c.rotate180;
    a.dets = e->dets_dev + (size_t)first * c.max_det;
    a.max_det = c.max_det;
    a.num_dets = reinterpret_cast<const int *>(e->fout_dev + first);
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.n_boxes = 0;
    a.boxes = nullptr;
    a.labels = e->light_labels + (size_t)first * e->light_pool;
    a.label_pool = e->light_pool;
    a.points = e->light_points + (size_t)first * c.max_det * kLightPointsCap * 2;
    a.points_cap = kLightPointsCap;
    a.hulls = e->light_hulls + (size_t)first * c.max_det * kLightPointsCap * 4;
    a.binary_threshold = c.binary_threshold;
    a.light_min_ratio = c.light_min_ratio; a.light_max_ratio = c.light_max_ratio; a.light_max_angle = c.light_max_angle;
    a.min_small_cd = c.armor_min_small_center_distance; a.max_small_cd = c.armor_max_small_center_distance;
    a.min_large_cd = c.armor_min_large_center_distance; a.max_large_cd = c.armor_max_large_center_distance;
    a.pnp = e->pnp_dev;
    a.first = first; a.pnp_stride = e->post.pnp_stride;
    a.pnp_armor_size = c.armor_size;
    return a;
}

static BayerArgs bayer_args(const irmv_engine *e, int first)   // a Bayer engine's demosaic of its raw slots from `first` on
{
    BayerArgs a = e->bayer;
    a.raw = e->raw_dev + (size_t)first * e->src_bytes; a.dst = (e->window ? e->full_dev : e->src_dev) + (size_t)first * e->full_bytes;
    return a;
}

static void launch_bayer(const irmv_engine *e, int first, int count, hipStream_t s)
{
    if (e->bayer_table) launch_demosaic_table(bayer_args(e, first), e->isp_table_dev, e->bayer_mhc, count, s);
    else launch_demosaic(bayer_args(e, first), count, s);
}

// The crop of slots [first, first + count): out of their device frames, or (pinned) out of the pinned slots themselves.
static void launch_crop(const irmv_engine *e, int first, int count, bool pinned, hipStream_t s)
{
    CropArgs a{};
    a.src = pinned ? e->src_host_dev : e->full_dev; a.src_slot_bytes = e->full_bytes;
    a.dst = e->src_dev; a.dst_slot_bytes = e->frame_bytes;
    a.win = e->win_dev; a.first = first;
    a.full_w = e->full_w; a.full_h = e->full_h; a.win_w = e->cfg.src_width; a.win_h = e->cfg.src_height;
    launch_window_crop(a, count, s);
}

static PostArgs post_args(const irmv_engine *e, int first)
{
    PostArgs p = e->post;
    p.head_all = e->head_all;
    p.slots_total = e->cfg.num_slots;
    p.first = first;
    p.boxes = e->boxes + (size_t)first * e->A * 4;
    p.keys = e->keys + (size_t)first * e->A * e->nc;
    p.key_cap = e->A * e->nc;
    p.dets = (e->zero_copy_results ? e->dets_host_dev : e->dets_dev) + (size_t)first * e->cfg.max_det;
    p.fout = (e->zero_copy_results ? e->fout_host_dev : e->fout_dev) + first;
    if (p.dbg) p.dbg += (size_t)first * 16;
    p.counts = e->split_scan ? e->cand_counts + first : nullptr;
    p.cand_bits = e->sparse_head ? e->cand_bits + (size_t)first * e->cand_words : nullptr;
    p.cand_words = e->cand_words;
    return p;
}

// one fused C2f block (OP_C2F32).  (A 16 x 16 tile on an 8-wave workgroup -- a third less halo work, one workgroup per CU --
// was built and measured in round 3: 5 - 30 % slower than the 8 x 16 tile in an eager replay, a tie in the benchmarked one;
// dropped.)
static bool launch_c2f32_op(const irmv_engine *e, const Op &op, int first, int count, hipStream_t s)
{
    C2f32Args a{};
    const Tensor &ct = e->tensors[op.res_t];
    const Tensor &ot = e->tensors[op.out_t];
    if (op.sub[0] >= 0) {
        ConvArgs ca;
        fill_conv_args(e, e->ops[op.sub[0]], first, count, ca, false);
        a.s0 = ca.s0; a.s1 = ca.s1; a.cin1 = ca.Cin;
        a.w_cv1 = e->ops[op.sub[0]].w_packed; a.b_cv1 = e->ops[op.sub[0]].bias;
    } else {
        a.cin1 = 32;
    }
    a.cat = static_cast<half_t *>(ct.slot(first)); a.cat_ld = ct.C; a.prev_coff = 64;
    a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
    a.H = op.Hin; a.W = op.Win;
    a.tiles_x = (op.Win + kC2f32TileW - 1) / kC2f32TileW; a.tiles_y = (op.Hin + kC2f32TileH - 1) / kC2f32TileH;
    a.w_m1 = e->ops[op.sub[1]].w_packed; a.b_m1 = e->ops[op.sub[1]].bias;
    a.w_m2 = e->ops[op.sub[2]].w_packed; a.b_m2 = e->ops[op.sub[2]].bias;
    if (op.sub[3] >= 0) { a.w_cv2 = e->ops[op.sub[3]].w_packed; a.b_cv2 = e->ops[op.sub[3]].bias; }
    return launch_c2f32(op.mode, op.shortcut, a, count, s);
}

// The kernels of the graph's non-conv layer ops (depthwise, shuffle, model.0.conv, SPPF) on slots [first, first + count):
// what a step launches for them, and what irmv_engine_run_op runs.
static void launch_graph_op(irmv_engine *e, const Op &op, int first, int count, hipStream_t s)
{
    switch (op.kind) {
    case OP_DW: {
        DwArgs a;
        const Tensor &xt = e->tensors[op.s0.t], &ot = e->tensors[op.out_t];
        a.x = static_cast<const half_t *>(xt.slot(first)) + op.s0.coff; a.x_ld = xt.C;
        a.y = static_cast<half_t *>(ot.slot(first)) + op.out_coff; a.y_ld = ot.C;
        a.w = op.w_packed; a.b = op.bias;
        a.Hin = op.Hin; a.Win = op.Win; a.Hout = op.Hout; a.Wout = op.Wout; a.C = op.cout; a.stride = op.cfg.stride;
        launch_dwconv3x3(a, count, s);
        break;
    }
    case OP_SHUF: {
        ShufArgs a;
        const Tensor &at = e->tensors[op.s0.t], &bt = e->tensors[op.s1.t], &ot = e->tensors[op.out_t];
        a.a = static_cast<const half_t *>(at.slot(first)) + op.s0.coff; a.a_ld = at.C;
        a.b = static_cast<const half_t *>(bt.slot(first)) + op.s1.coff; a.b_ld = bt.C;
        a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
        a.bc = op.s0.C;
        a.pixels = (size_t)count * op.Hin * op.Win;
        launch_shuffle_cat(a, s);
        break;
    }
    case OP_CONV0: {
        Conv0Args a;
        a.x = static_cast<const half_t *>(e->tensors[op.s0.t].slot(first));
        a.y = static_cast<half_t *>(e->tensors[op.out_t].slot(first));
        a.w = e->conv0_w; a.b = e->conv0_b; a.net_w = e->cfg.net_size; a.net_h = e->cfg.net_height; a.batch = count;
        launch_conv0(a, s);
        break;
    }
    case OP_POOL: {
        const Tensor &t = e->tensors[op.out_t];
        launch_sppf_pool(static_cast<half_t *>(t.slot(first)), count, t.H, t.W, t.C / 4, s);
        break;
    }
    default: break;
    }
}

// Enqueue a step of kind `kind` on slots [first, first + count), stream s: the launches of e->plans[kind], in order.
// ev != nullptr (irmv_engine_profile): one event pair per launch, around `reps` repetitions of it (one if it is `once`).
static int enqueue_step(irmv_engine *e, StepKind kind, int first, int count, hipStream_t s, int reps, std::vector<EvRec> *ev, bool crop_pinned = false)
{
    const int net_w = e->cfg.net_size, net_h = e->cfg.net_height;
    const PostArgs pa = post_args(e, first);
    for (const Launch &l : e->plans[kind]) {
        const Op &op = e->ops[l.op];
        EvRec r{};
        if (ev) {
            HIP_TRY(hipEventCreate(&r.a));
            HIP_TRY(hipEventCreate(&r.b));
            HIP_TRY(hipEventRecord(r.a, s));
        }
        const int n = l.once ? 1 : reps;
        for (int rep = 0; rep < n; rep++)
        switch (op.kind) {
        case OP_DEMOSAIC: launch_bayer(e, first, count, s); break;
        case OP_CROP: launch_crop(e, first, count, crop_pinned, s); break;
        case OP_PRE: {
            PreArgs a;
            a.src = e->src_dev + (size_t)first * e->frame_bytes;
            a.dst = static_cast<half_t *>(e->tensors[op.out_t].slot(first));
            a.tx = e->tap_x; a.ty = e->tap_y;
            a.sw = e->cfg.src_width; a.sh = e->cfg.src_height; a.net_w = net_w; a.net_h = net_h; a.swap_rb = e->cfg.swap_rb;
            a.src_slot_bytes = e->frame_bytes;
            launch_preprocess(a, count, s);
            break;
        }
        case OP_FRONT: {
            FrontArgs a;
            a.src = e->src_dev + (size_t)first * e->frame_bytes;
            a.src_slot_bytes = e->frame_bytes;
            a.tx = e->tap_x; a.ty = e->tap_y;
            a.vx0 = e->front_v[0]; a.vx1 = e->front_v[1]; a.vy0 = e->front_v[2]; a.vy1 = e->front_v[3];
            a.sw = e->cfg.src_width; a.sh = e->cfg.src_height; a.net_w = net_w; a.net_h = net_h; a.swap_rb = e->cfg.swap_rb;
            a.fastx = e->front_fastx; a.fx_i0 = e->front_fx_i0; a.fx_step = e->front_fx_step;
            a.w0 = e->conv0_w; a.b0 = e->conv0_b;
            a.w1 = op.w_packed; a.b1 = op.bias;
            const Tensor &ot = e->tensors[op.out_t];
            a.out = static_cast<half_t *>(ot.slot(first));
            a.out_ld = ot.C;
            a.tiles_x = e->front_tiles_x; a.tiles_y = e->front_tiles_y; a.tile_y = e->front_tile_y;
            a.stage_bytes = e->front_stage_bytes;
            if (!launch_front(a, count, s)) return fail(IRMV_ERR_HIP, "fused front kernel: LDS request refused");
            break;
        }
        case OP_C2F2: {
            C2fArgs a;
            const Tensor &xt = e->tensors[op.s0.t], &ot = e->tensors[op.out_t];
            a.x = static_cast<const half_t *>(xt.slot(first)); a.x_ld = xt.C;
            a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
            a.H = xt.H; a.W = xt.W;
            a.tiles_x = (xt.W + kC2fTile - 1) / kC2fTile; a.tiles_y = (xt.H + kC2fTile - 1) / kC2fTile;
            const Op &c1 = e->ops[op.sub[0]], &m1 = e->ops[op.sub[1]], &m2 = e->ops[op.sub[2]], &c2 = e->ops[op.sub[3]];
            a.w_cv1 = c1.w_packed; a.w_m1 = m1.w_packed; a.w_m2 = m2.w_packed; a.w_cv2 = c2.w_packed;
            a.b_cv1 = c1.bias; a.b_m1 = m1.bias; a.b_m2 = m2.bias; a.b_cv2 = c2.bias;
            launch_c2f2(a, count, s);
            break;
        }
        case OP_C2F32: if (!launch_c2f32_op(e, op, first, count, s)) return fail(IRMV_ERR_ARG, "no fused C2f kernel for " + op.layer); break;
        case OP_BNECK: {
            const Op &m1 = e->ops[op.sub[0]], &m2 = e->ops[op.sub[1]];
            const Tensor &ct = e->tensors[op.res_t];
            BneckArgs a{};
            a.yin = static_cast<const half_t *>(ct.slot(first)) + m1.s0.coff; a.yin_ld = ct.C;
            a.ynext = static_cast<half_t *>(ct.slot(first)) + m2.out_coff; a.ynext_ld = ct.C;
            a.cat = static_cast<const half_t *>(ct.slot(first)); a.cat_ld = ct.C;
            a.H = op.Hin; a.W = op.Win;
            a.tiles_x = (op.Win + kBneckTile - 1) / kBneckTile; a.tiles_y = (op.Hin + kBneckTile - 1) / kBneckTile;
            a.w_m1 = m1.w_lds[0]; a.b_m1 = m1.bias; a.w_m2 = m2.w_lds[0]; a.b_m2 = m2.bias;
            int ks2 = 6;
            if (op.sub[2] >= 0) {
                const Op &c2 = e->ops[op.sub[2]];
                const Tensor &ot = e->tensors[c2.out_t];
                a.out = static_cast<half_t *>(ot.slot(first)) + c2.out_coff; a.out_ld = ot.C;
                a.w_cv2 = c2.w_packed; a.b_cv2 = c2.bias;
                ks2 = c2.ksteps;
            }
            if (!launch_bneck64(op.mode, ks2, op.shortcut, a, count, s)) return fail(IRMV_ERR_ARG, "no fused bottleneck kernel for " + op.layer);
            break;
        }
        case OP_KPT3: {
            const Op &o0 = e->ops[op.sub[0]], &o1 = e->ops[op.sub[1]], &o2 = e->ops[op.sub[2]];
            const Tensor &xt = e->tensors[o0.s0.t], &ht = e->tensors[o2.out_t];
            Kpt3Args a{};
            a.x = static_cast<const half_t *>(xt.slot(first)) + o0.s0.coff; a.x_ld = xt.C;
            a.H = op.Hin; a.W = op.Win;
            a.tiles_x = (op.Win + kKpt3Tile - 1) / kKpt3Tile; a.tiles_y = (op.Hin + kKpt3Tile - 1) / kKpt3Tile;
            a.w1 = o0.w_lds[0]; a.b1 = o0.bias;
            a.w2 = o1.w_packed; a.b2 = o1.bias;
            a.w3 = o2.w_k16; a.b3 = o2.bias;
            a.out = static_cast<float *>(ht.slot(first)) + o2.out_coff; a.out_ld = ht.C;
            if (l.sparse) { a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words; a.abase = e->lvl_base[op.level]; a.tile_gate = l.gate; }
            if (!launch_kpt3(a, op.cin, count, s)) return fail(IRMV_ERR_ARG, "no fused keypoint-branch kernel for " + op.layer);
            break;
        }
        case OP_DW: case OP_SHUF: case OP_CONV0: case OP_POOL: launch_graph_op(e, op, first, count, s); break;
        case OP_CONV: {
            unsigned scan = rep == n - 1 ? l.scan : 0u;   // (a profiled launch is repeated: only its last repetition appends candidates)
            // ... with the sparse head the other repetitions still run the step's kernel -- no class store --, behind a threshold
            // no logit passes: no key, no bit
            PostArgs pr = pa;
            if (!scan && l.scan && e->sparse_head) { scan = l.scan; pr.logit_thr = INFINITY; }
            if (l.group >= 0) {
                if (!launch_head_group(e, e->head_groups[l.group], first, &pr, scan, s)) return fail(IRMV_ERR_ARG, "grouped launch refused: " + l.name);
                break;
            }
            ConvArgs a;
            fill_conv_args(e, op, first, count, a, l.fused);
            if (scan) scan_args_for(e, op, pr, a);
            if (l.sparse || l.gate) { a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words; a.scan_abase = e->lvl_base[op.level]; a.tile_gate = l.gate; }
            if (!run_conv(op, l.cfg_one ? op.cfg_one : op.cfg, a, count, s)) return fail(IRMV_ERR_ARG, std::string("no conv kernel for ") + op.kname + " (" + op.layer + ")");
            break;
        }
        case OP_SCAN: launch_scan_decode(pa, count, s); break;
        case OP_NMS: { PostArgs pn = pa; pn.keys_only = l.keys_only ? 1 : 0; launch_nms_pnp(pn, count, s); break; }
        case OP_LIGHT: launch_light_extract(light_args(e, first), e->cfg.max_det, count, s); break;
        }
        HIP_TRY(hipGetLastError());
        if (ev) {
            HIP_TRY(hipEventRecord(r.b, s));
            ev->push_back(r);
        }
    }
    return IRMV_OK;
}

// Frame upload and result download: plain async copies, pinned memory both ways, on the streams submit_group() picks.
// bands (never inside a stream capture, whose copy parameters are baked): an HWC window engine moves, for groups of up to 8
// slots, only the band of full-width rows each slot's window covers -- one 1-D copy per slot, to the same offset of its device frame.
constexpr int kBandUploadMaxSlots = 8;
static int copy_in(irmv_engine *e, int first, int count, hipStream_t st, bool bands = false)
{
    if (bands && e->window && !e->raw_dev && count <= kBandUploadMaxSlots) {
        const size_t pitch = (size_t)e->full_w * 3, len = (size_t)e->cfg.src_height * pitch;
        for (int s = first; s < first + count; s++) {
            const int by0 = e->cfg.rotate180 ? e->full_h - e->win_org[s].y - e->cfg.src_height : e->win_org[s].y;
            const size_t off = (size_t)s * e->src_bytes + (size_t)by0 * pitch;
            HIP_TRY(hipMemcpyAsync(e->full_dev + off, e->src_host + off, len, hipMemcpyHostToDevice, st));
        }
        return IRMV_OK;
    }
    HIP_TRY(hipMemcpyAsync(upload_dev(e) + (size_t)first * e->src_bytes, e->src_host + (size_t)first * e->src_bytes,
                           e->src_bytes * count, hipMemcpyHostToDevice, st));
    return IRMV_OK;
}

// One or two frames travel from the pinned slots as a KERNEL (k_pre.hip upload_frame_kernel), larger groups on the copy engine.
static bool upload_as_kernel(const irmv_engine *e, int first, int count)
{
    return count <= 2 && e->upload_kernel_blocks > 0 && e->src_host_dev && upload_aligned(e->src_bytes, first, count);
}

// The synchronous upload of slots [first, first + count) on stream st.  (A Bayer engine's single-frame upload stays a kernel
// of its own in front of the demosaic: the demosaic reading the pinned slot itself was built and measured slower, DESIGN.md
// section 9.)
// An HWC window engine's synchronous step of one or two slots uploads nothing: its crop reads the window out of the pinned
// slots (crop_from_pinned), so only the window crosses PCIe.  `captured`: the copy becomes a graph node (whole frames).
static bool crop_from_pinned(const irmv_engine *e, int count)
{
    return e->window && !e->raw_dev && e->window_upload && count <= 2 && e->upload_kernel_blocks > 0 && e->src_host_dev;
}

static int upload_sync(irmv_engine *e, int first, int count, hipStream_t st, bool captured)
{
    if (crop_from_pinned(e, count)) return IRMV_OK;
    if (!upload_as_kernel(e, first, count)) return copy_in(e, first, count, st, !captured);
    const size_t off = (size_t)first * e->src_bytes;
    launch_upload_frames(e->src_host_dev + off, upload_dev(e) + off, e->src_bytes * count, e->upload_kernel_blocks, st);
    return IRMV_OK;
}

static int copy_out(irmv_engine *e, int first, int count, hipStream_t st = nullptr)
{
    if (!st) st = e->stream;
    if (e->zero_copy_results) return IRMV_OK;   // the kernel has already written the pinned records
    HIP_TRY(hipMemcpyAsync(e->dets_host + (size_t)first * e->cfg.max_det, e->dets_dev + (size_t)first * e->cfg.max_det,
                           (size_t)count * e->cfg.max_det * sizeof(DevDet), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(e->fout_host + first, e->fout_dev + first, (size_t)count * sizeof(DevFrameOut),
                           hipMemcpyDeviceToHost, st));
    return IRMV_OK;
}

static int check_range(const irmv_engine *e, int first, int count)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (first < 0 || count < 1 || first + count > e->cfg.num_slots) return fail(IRMV_ERR_ARG, "slot range out of bounds");
    return IRMV_OK;
}

static int get_graph(irmv_engine *e, StepKind kind, int first, int count, bool upload, hipGraphExec_t *out)
{
    const GraphKey key{first, count, kind, upload};
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) { *out = it->second; return IRMV_OK; }
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int rc = IRMV_OK;
    if (upload)   // the frames' upload as the graph's first node (synchronous single-stream submits): one or two frames as a kernel
        rc = upload_sync(e, first, count, e->stream, true);
    if (!rc) rc = enqueue_step(e, kind, first, count, e->stream, 1, nullptr, upload && crop_from_pinned(e, count));
    hipError_t ce = hipStreamEndCapture(e->stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (ce != hipSuccess) return fail(IRMV_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    hipGraphExec_t ge = nullptr;
    HIP_TRY(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    e->graphs[key] = ge;
    *out = ge;
    return IRMV_OK;
}

static int group_of(irmv_engine *e, int first, int count, SlotGroup **out)
{
    const auto key = std::make_pair(first, count);
    auto it = e->groups.find(key);
    if (it == e->groups.end()) {
        SlotGroup g;
        g.first = first; g.count = count;
        HIP_TRY(hipEventCreateWithFlags(&g.h2d, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.out, hipEventDisableTiming));
        it = e->groups.emplace(key, g).first;
    }
    *out = &it->second;   // std::map nodes never move
    return IRMV_OK;
}

// One slot group: [upload] -> ONE hipGraph -> download of the results, in order on compute stream `st`.
//
// IRMV_SUBMIT_ASYNC_UPLOAD moves the upload to the engine's upload stream (the dGPU form of the
// reference's TripleBuffer, include/irmv_detection/triple_buffer.hpp:24-40, whose slots ARE the engines' input memory):
//
//   upload stream    [wait: this group's previous step is done with its device frames]  H2D frames  -> ev h2d
//   compute stream   [wait: ev h2d]  hipGraph, D2H results                                           -> ev out
//
// so group B's frames cross PCIe while group A's kernels run.  The price is one cross-stream event hop per group
// (measured on this stack: scripts/probes/stream_probe.cpp), which is why a lone synchronous detect() -- nothing to
// overlap with -- keeps everything on one stream, and why the (tiny) download never leaves the compute stream.
static int submit_group(irmv_engine *e, int f, int c, uint32_t flags, hipStream_t st)
{
    const bool async_up = (flags & IRMV_SUBMIT_H2D) && (flags & IRMV_SUBMIT_ASYNC_UPLOAD) && !e->inline_copies;
    // An upload that rides the compute stream anyway (the synchronous detect()) is captured INTO the step's graph: one
    // submission instead of two, and the copy -> first kernel hand-over is the graph's own (IRMV_GRAPH_UPLOAD=0: a separate
    // hipMemcpyAsync in front of the graph, as before; same bits)
    // A synchronous single-frame step (the reference's detect(), src/yolo_engine.cpp:153-177) has two launch forms with the same
    // kernels and the same bits: ONE hipGraph replay, or its 41 launches issued one by one behind the upload (round 5: a graph
    // replay spends ~10 us of host work before its first packet reaches the GPU, a direct launch ~4; with the 70 us upload in
    // front the host stays far ahead of the GPU: 0.339 -> 0.331 ms per 1280 x 1024 frame).  Every other step is a graph replay.
    const bool eager = e->sync_launch == 1 && c == 1 && (flags & IRMV_SUBMIT_H2D) && !async_up;
    const bool pinned = (flags & IRMV_SUBMIT_H2D) && !async_up && crop_from_pinned(e, c);   // (no upload at all: nothing to keep out of the graph)
    const bool graph_up = (flags & IRMV_SUBMIT_H2D) && !async_up && (e->graph_upload || pinned) && !eager;
    const StepKind kind = c == 1 ? STEP_ONE : STEP_BATCH;
    hipGraphExec_t ge = nullptr;
    if (!eager) TRY(get_graph(e, kind, f, c, graph_up, &ge));
    SlotGroup *g;
    TRY(group_of(e, f, c, &g));
    hipStream_t up = async_up ? e->h2d_stream : st;
    // slots last used through a different grouping: order behind that group's completion
    SlotGroup *seen[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int s = f; s < f + c; s++) {
        SlotGroup *o = e->slot_owner[s];
        e->slot_owner[s] = g;
        if (!o || o == g || !o->in_flight || o == seen[0] || o == seen[1] || o == seen[2] || o == seen[3]) continue;
        seen[3] = seen[2]; seen[2] = seen[1]; seen[1] = seen[0]; seen[0] = o;
        if (o->compute != st) HIP_TRY(hipStreamWaitEvent(st, o->out, 0));
        if (up != st) HIP_TRY(hipStreamWaitEvent(up, o->out, 0));
    }
    if (g->in_flight && g->compute != st) HIP_TRY(hipStreamWaitEvent(st, g->out, 0));   // the group moved to another compute stream
    if (flags & IRMV_SUBMIT_H2D) {
        if (async_up) {
            if (g->in_flight) HIP_TRY(hipStreamWaitEvent(up, g->out, 0));   // previous step has consumed the device frames
            TRY(copy_in(e, f, c, up, true));
            HIP_TRY(hipEventRecord(g->h2d, up));
            HIP_TRY(hipStreamWaitEvent(st, g->h2d, 0));
        } else if (!graph_up) {
            // (an eager step, or IRMV_GRAPH_UPLOAD=0)
            TRY(upload_sync(e, f, c, st, false));
        }
    }
    if (eager) TRY(enqueue_step(e, kind, f, c, st, 1, nullptr, pinned));
    else HIP_TRY(hipGraphLaunch(ge, st));
    if (e->sparse_head) std::fill(e->head_stale.begin() + f, e->head_stale.begin() + f + c, 1);
    if (e->sparse_branch) std::fill(e->branch_stale.begin() + f, e->branch_stale.begin() + f + c, 1);
    if (e->window) std::copy(e->win_org.begin() + f, e->win_org.begin() + f + c, e->sub_org.begin() + f);   // what these results are shifted by
    TRY(copy_out(e, f, c, st));
    HIP_TRY(hipEventRecord(g->out, st));
    g->in_flight = true;
    g->async_up = async_up;
    g->compute = st;
    return IRMV_OK;
}

extern "C" int irmv_engine_submit(irmv_engine *e, int first, int count, uint32_t flags)
{
    TRY(check_range(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    // A multi-slot step is cut into num_streams independent sub-batches, one captured graph each, on
    // separate streams: while one sub-batch sits in a launch gap or a kernel tail the other keeps the
    // CUs busy (two sub-batches measured +30 % frames/s over one stream at 32 frames).
    int share = count > 1 ? stream_share(e, count) : count;
    // Single-slot steps ride the compute stream of their slot (slot mod num_streams): a single frame fills a fraction of
    // the chip, so the steps of two slots in flight (the TripleBuffer's depth) overlap instead of queueing behind each other.
    int si = count == 1 ? first % e->num_streams : 0;
    // A submit of exactly ONE stream's share of the engine's slots, aligned to it, is that share's sub-batch of a whole-engine
    // step: the same captured graph on the same stream.  A caller that feeds the shares separately decides itself how far
    // apart the streams run (two shares started together execute the same kernel at the same time all the way down).
    const int full_share = stream_share(e, e->cfg.num_slots);
    if (count > 1 && count == full_share && first % full_share == 0 && first / full_share < e->num_streams) { share = count; si = first / full_share; }
    for (int f = first; f < first + count; f += share, si++) {
        const int c = std::min(share, first + count - f);
        hipStream_t st = si == 0 ? e->stream : e->extra_streams[si - 1];
        TRY(submit_group(e, f, c, flags, st));
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_wait(irmv_engine *e);

extern "C" int irmv_engine_debug_poke_candidate_counts(irmv_engine *e, int value)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->cand_counts) return fail(IRMV_ERR_ARG, "this engine keeps no candidate counters");
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    std::vector<int> v((size_t)e->cfg.num_slots, value);
    HIP_TRY(hipMemcpy(e->cand_counts, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_debug_read_cand_bits(irmv_engine *e, int slot, uint32_t *words, int cap, int *n, int *sparse)
{
    TRY(check_range(e, slot, 1));
    if (!n || !sparse) return fail(IRMV_ERR_ARG, "n / sparse is null");
    *sparse = e->sparse_head ? 1 : 0;
    *n = e->sparse_head ? e->cand_words : 0;
    if (!words || *n == 0) return IRMV_OK;
    if (cap < *n) return fail(IRMV_ERR_ARG, "read_cand_bits: buffer too small");
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpy(words, e->cand_bits + (size_t)slot * e->cand_words, (size_t)e->cand_words * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return IRMV_OK;
}

static int ensure_dense_head(irmv_engine *e, int slot);

extern "C" int irmv_engine_run_post(irmv_engine *e, int first, int count)
{
    TRY(check_range(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    for (int s = first; s < first + count; s++) TRY(ensure_dense_head(e, s));   // (scan_decode_kernel reads every anchor's class logits)
    hipGraphExec_t ge;
    TRY(get_graph(e, STEP_POST, first, count, false, &ge));
    HIP_TRY(hipGraphLaunch(ge, e->stream));
    TRY(copy_out(e, first, count));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

extern "C" int irmv_engine_wait(irmv_engine *e)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(e->h2d_stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 1; i < e->num_streams; i++) HIP_TRY(hipStreamSynchronize(e->extra_streams[i - 1]));
    for (auto &kv : e->groups) kv.second.in_flight = false;
    return IRMV_OK;
}

// Block until the pinned slots [first, first + count) have been read by their last submit's upload: from then on a producer
// may overwrite them (the moment the TripleBuffer's consumer can give the buffer back), while the kernels still run.
extern "C" int irmv_engine_wait_upload(irmv_engine *e, int first, int count)
{
    TRY(check_range(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    SlotGroup *last = nullptr;
    for (int s = first; s < first + count; s++) {
        SlotGroup *o = e->slot_owner[s];
        if (!o || o == last || !o->in_flight) continue;
        // an upload on the side stream has its own event; an inline upload is ordered in front of the kernels, so the
        // group's completion event covers it
        HIP_TRY(hipEventSynchronize(o->async_up ? o->h2d : o->out));
        last = o;
    }
    return IRMV_OK;
}

// Block until the results of slots [first, first + count) from their last submit are host-visible; other slots may
// stay in flight (the consumer side of the TripleBuffer: take the newest finished slot while the next one runs).
extern "C" int irmv_engine_wait_slots(irmv_engine *e, int first, int count)
{
    TRY(check_range(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    SlotGroup *last = nullptr;
    for (int s = first; s < first + count; s++) {
        SlotGroup *o = e->slot_owner[s];
        if (!o || o == last || !o->in_flight) continue;
        HIP_TRY(hipEventSynchronize(o->out));
        // the whole group is done only if this call covers it; otherwise it merely stays marked in flight (harmless)
        if (o->first >= first && o->first + o->count <= first + count) o->in_flight = false;
        last = o;
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_results(irmv_engine *e, int slot, irmv_det *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    const DevFrameOut &fo = e->fout_host[slot];
    const int k = std::min(fo.num_dets, cap);
    const DevDet *d = e->dets_host + (size_t)slot * e->cfg.max_det;
    // device records are window-local: the corner the slot was submitted with brings them to full-frame coordinates
    const float ox = e->window ? (float)e->sub_org[slot].x : 0.f, oy = e->window ? (float)e->sub_org[slot].y : 0.f;
    for (int i = 0; i < k; i++) {
        irmv_det &o = out[i];
        memcpy(o.xyxy, d[i].xyxy, 16);
        o.score = d[i].score;
        // magic_enum::enum_cast<ArmorClass>(label).value_or(UNKNOWN), src/yolo_engine.cpp:216
        o.class_id = (d[i].cls >= 0 && d[i].cls < IRMV_NUM_CLASSES) ? d[i].cls : IRMV_NUM_CLASSES;
        o.anchor = d[i].anchor;
        o.pnp_ok = d[i].pnp_ok;
        memcpy(o.kpts, d[i].kpts, 32);
        memcpy(o.rvec, d[i].rvec, 24);
        memcpy(o.tvec, d[i].tvec, 24);
        memcpy(o.quat, d[i].quat, 32);
        o.armor_valid = d[i].armor_valid;
        o.armor_size = d[i].armor_size;
        o.n_lights = d[i].n_lights;
        o.reserved = 0;
        if (e->window) {
            for (int j = 0; j < 4; j++) o.xyxy[j] += (j & 1) ? oy : ox;
            for (int j = 0; j < 8; j++) o.kpts[j] += (j & 1) ? oy : ox;
        }
    }
    *n = k;
    return IRMV_OK;
}

extern "C" int irmv_engine_detect(irmv_engine *e, int slot, irmv_det *out, int cap, int *n)
{
    const auto t0 = std::chrono::high_resolution_clock::now();
    // a synchronous single-slot call has nothing to overlap with: upload, graph and download ride ONE stream
    TRY(irmv_engine_submit(e, slot, 1, IRMV_SUBMIT_H2D));
    TRY(irmv_engine_wait_slots(e, slot, 1));
    const int rc = irmv_engine_results(e, slot, out, cap, n);
    e->last_detect_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    return rc;
}

extern "C" double irmv_engine_last_detect_ms(const irmv_engine *e) { return e ? e->last_detect_ms : 0.0; }

// The slot's pinned frame -> its HWC device frame (src_dev) on stream st, outside a step: an HWC engine copies it there, a
// Bayer engine copies the raw frame to its device raw slot and demosaics it; a window engine then cuts the slot's window out.
static int load_frame(irmv_engine *e, int slot, hipStream_t st)
{
    TRY(copy_in(e, slot, 1, st, true));
    if (e->raw_dev) {
        launch_bayer(e, slot, 1, st);
        HIP_TRY(hipGetLastError());
    }
    if (e->window) {
        launch_crop(e, slot, 1, false, st);
        HIP_TRY(hipGetLastError());
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_rotated_image(irmv_engine *e, int slot, uint8_t *dst)
{
    TRY(check_range(e, slot, 1));
    if (!dst) return fail(IRMV_ERR_ARG, "dst is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(load_frame(e, slot, e->stream));
    launch_rotate180(e->src_dev + (size_t)slot * e->frame_bytes, e->rot_dev, e->cfg.src_width, e->cfg.src_height, e->stream);
    HIP_TRY(hipMemcpyAsync(dst, e->rot_dev, e->frame_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

static_assert(sizeof(irmv_light_rec) == sizeof(LightTraceRec) && sizeof(irmv_light_trace) == sizeof(LightTrace) &&
                  offsetof(irmv_light_trace, starts) == offsetof(LightTrace, starts) && offsetof(irmv_light_trace, points) == offsetof(LightTrace, points) &&
                  offsetof(irmv_light_trace, recs) == offsetof(LightTrace, recs) && offsetof(irmv_light_rec, length) == offsetof(LightTraceRec, length) &&
                  IRMV_LIGHT_MAX_CONTOURS == kLightMaxContours && IRMV_LIGHT_POINTS_CAP == kLightPointsCap,
              "irmv_light_trace is LightTrace");

// irmv_engine_extract_armors; trace != nullptr: irmv_engine_light_trace (the kernel also records its stages)
static int extract_armors(irmv_engine *e, int slot, const float *xyxy, int n, irmv_light_trace *trace, irmv_det *out)
{
    TRY(check_range(e, slot, 1));
    if (n < 0 || n > e->cfg.max_det || (n > 0 && (!xyxy || !out))) return fail(IRMV_ERR_ARG, "n must be 0..max_det with xyxy/out set");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    hipStream_t st = e->stream;
    if (trace && !e->light_trace_dev) TRY(dev_alloc(e, (void **)&e->light_trace_dev, (size_t)e->cfg.max_det * sizeof(LightTrace)));
    if (trace) HIP_TRY(hipMemsetAsync(e->light_trace_dev, 0, (size_t)n * sizeof(LightTrace), st));
    TRY(load_frame(e, slot, st));
    // a window engine takes the boxes in full result coordinates: window-local for the kernel, the corner back onto its points
    const float ox = e->window ? (float)e->win_org[slot].x : 0.f, oy = e->window ? (float)e->win_org[slot].y : 0.f;
    std::vector<float> local;
    if (e->window) {
        local.assign(xyxy, xyxy + (size_t)n * 4);
        for (size_t j = 0; j < local.size(); j++) local[j] -= (j & 1) ? oy : ox;
        HIP_TRY(hipMemcpyAsync(e->light_boxes, local.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));   // (`local` is pageable memory of this call)
    } else {
        HIP_TRY(hipMemcpyAsync(e->light_boxes, xyxy, (size_t)n * 16, hipMemcpyHostToDevice, st));
    }
    LightArgs a = light_args(e, slot);
    a.dets = e->light_dets_dev;
    a.labels = e->light_labels;
    a.points = e->light_points;
    a.hulls = e->light_hulls;
    a.num_dets = nullptr;
    a.n_boxes = n;
    a.boxes = e->light_boxes;
    a.trace = trace ? e->light_trace_dev : nullptr;
    launch_light_extract(a, n, 1, st);
    HIP_TRY(hipGetLastError());
    if (trace) HIP_TRY(hipMemcpyAsync(trace, e->light_trace_dev, (size_t)n * sizeof(LightTrace), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(e->light_dets_host, e->light_dets_dev, (size_t)n * sizeof(DevDet), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        const DevDet &d = e->light_dets_host[i];
        irmv_det &o = out[i];
        memset(&o, 0, sizeof o);
        memcpy(o.xyxy, xyxy + 4 * i, 16);
        o.class_id = IRMV_NUM_CLASSES;
        o.pnp_ok = d.pnp_ok;
        memcpy(o.kpts, d.kpts, 32);
        if (e->window)
            for (int j = 0; j < 8; j++) o.kpts[j] += (j & 1) ? oy : ox;
        memcpy(o.rvec, d.rvec, 24);
        memcpy(o.tvec, d.tvec, 24);
        memcpy(o.quat, d.quat, 32);
        o.armor_valid = d.armor_valid;
        o.armor_size = d.armor_size;
        o.n_lights = d.n_lights;
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_extract_armors(irmv_engine *e, int slot, const float *xyxy, int n, irmv_det *out)
{
    return extract_armors(e, slot, xyxy, n, nullptr, out);
}

extern "C" int irmv_engine_light_trace(irmv_engine *e, int slot, const float *xyxy, int n, irmv_light_trace *trace, irmv_det *out)
{
    if (n > 0 && !trace) return fail(IRMV_ERR_ARG, "trace is null");
    return extract_armors(e, slot, xyxy, n, trace, out);
}

extern "C" int irmv_light_limits(int32_t out[4])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    out[0] = kLightMaxContours; out[1] = kLightPointsCap; out[2] = kLightLdsImage; out[3] = kLightLdsPoints;
    return IRMV_OK;
}

static int debug_lds_geometry(int *workgroups)
{
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    *workgroups = debug_lds_workgroups(cus);
    return IRMV_OK;
}

extern "C" int irmv_debug_lds_fill(uint32_t pattern32)
{
    int wgs = 0;
    if (int rc = debug_lds_geometry(&wgs)) return rc;
    uint32_t *d = nullptr, bad = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMalloc(&d, sizeof(uint32_t)));
    hipError_t e = hipMemset(d, 0, sizeof(uint32_t));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = launch_lds_fill(pattern32, d, wgs, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&bad, d, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(e);
    if (bad) return fail(IRMV_ERR_HIP, "irmv_debug_lds_fill: a workgroup read back something else than it wrote");
    return IRMV_OK;
}

extern "C" int irmv_debug_lds_probe(uint32_t pattern32, uint32_t word, uint32_t *out, int cap, int *n)
{
    static_assert(IRMV_DEBUG_LDS_WORDS == kDebugLdsWords, "header and kernel disagree");
    if (!n) return fail(IRMV_ERR_ARG, "n is null");
    int wgs = 0;
    if (int rc = debug_lds_geometry(&wgs)) return rc;
    *n = wgs;
    if (!out) return IRMV_OK;
    if (cap < wgs) return fail(IRMV_ERR_ARG, "cap is smaller than the number of workgroups");
    if (word >= (uint32_t)kDebugLdsWords) return fail(IRMV_ERR_ARG, "word is outside the workgroup's allocation");
    uint32_t *d = nullptr;
    const size_t bytes = (size_t)wgs * 4 * sizeof(uint32_t);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMalloc(&d, bytes));
    hipError_t e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = launch_lds_probe(pattern32, word, d, wgs, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(e);
    return IRMV_OK;
}

extern "C" int irmv_engine_point_source(const irmv_engine *e)
{
    if (!e) return -1;
    return e->classical ? IRMV_POINTS_CLASSICAL : IRMV_POINTS_KEYPOINT_HEAD;
}

extern "C" int irmv_engine_set_extract_params(irmv_engine *e, int binary_threshold, float light_min_ratio, float light_max_ratio,
                                              float light_max_angle, const double cd[4])
{
    if (!e || !cd) return fail(IRMV_ERR_ARG, "null argument");
    if (binary_threshold < 0 || binary_threshold > 255) return fail(IRMV_ERR_ARG, "binary_threshold must be 0..255");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    irmv_engine_cfg &c = e->cfg;
    const bool same = c.binary_threshold == binary_threshold && c.light_min_ratio == light_min_ratio && c.light_max_ratio == light_max_ratio &&
                      c.light_max_angle == light_max_angle && c.armor_min_small_center_distance == cd[0] &&
                      c.armor_max_small_center_distance == cd[1] && c.armor_min_large_center_distance == cd[2] &&
                      c.armor_max_large_center_distance == cd[3];
    if (same) return IRMV_OK;
    c.binary_threshold = binary_threshold;
    c.light_min_ratio = light_min_ratio; c.light_max_ratio = light_max_ratio; c.light_max_angle = light_max_angle;
    c.armor_min_small_center_distance = cd[0]; c.armor_max_small_center_distance = cd[1];
    c.armor_min_large_center_distance = cd[2]; c.armor_max_large_center_distance = cd[3];
    // captured steps of the classical mode carry these values as kernel arguments: re-capture on next use
    if (e->classical) {
        for (auto &g : e->graphs) (void)hipGraphExecDestroy(g.second);
        e->graphs.clear();
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_set_bayer_isp(irmv_engine *e, const uint16_t gain_q8[3], const uint8_t *lut)
{
    if (!e || !gain_q8) return fail(IRMV_ERR_ARG, "engine / gain_q8 is null");
    if (!e->raw_dev) return fail(IRMV_ERR_ARG, "irmv_engine_set_bayer_isp: not a Bayer engine (src_format is IRMV_SRC_HWC8)");
    for (int i = 0; i < 3; i++)
        if (gain_q8[i] > 1023) return fail(IRMV_ERR_ARG, "gain_q8 must be in [0, 1023] (Q8, 256 = 1.0)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the table, no graph is running
    for (int i = 0; i < 3; i++) e->isp_gain[i] = e->cfg.bayer_gain_q8[i] = gain_q8[i];
    for (int i = 0; i < kBayerTableBytes; i++) e->isp_lut[i] = lut ? lut[i] : (uint8_t)(i & 255);
    TRY(write_isp_table(e));
    if (!e->bayer_table) {
        // From the argument-gain kernel to the table kernel: the captured steps hold the old kernel node, so they are dropped
        // and captured again on their next use (run_post's graphs have no demosaic node and stay).  Later sets only rewrite
        // the table, which the kernels read from device memory when they run.
        e->bayer_table = true;
        for (auto it = e->graphs.begin(); it != e->graphs.end();) {
            if (it->first.kind == STEP_POST) { ++it; continue; }
            (void)hipGraphExecDestroy(it->second);
            it = e->graphs.erase(it);
        }
        for (size_t i = 0; i < e->ops.size(); i++) {
            if (e->ops[i].kind != OP_DEMOSAIC) continue;
            snprintf(e->ops[i].kname, sizeof e->ops[i].kname, "%s", demosaic_kname(e));
            for (auto &plan : e->plans)
                for (Launch &l : plan)
                    if (l.op == (int)i) l.name = e->ops[i].kname;
        }
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_get_bayer_isp(const irmv_engine *e, uint16_t gain_q8[3], uint8_t *lut)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->raw_dev) return fail(IRMV_ERR_ARG, "irmv_engine_get_bayer_isp: not a Bayer engine (src_format is IRMV_SRC_HWC8)");
    if (gain_q8) for (int i = 0; i < 3; i++) gain_q8[i] = e->isp_gain[i];
    if (lut) memcpy(lut, e->isp_lut, kBayerTableBytes);
    return IRMV_OK;
}

// ---- read-backs --------------------------------------------------------------------
static int read_tensor_f32(irmv_engine *e, const Tensor &t, int slot, std::vector<float> &out)
{
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    out.resize(t.slot_elems);
    if (t.f32) {
        HIP_TRY(hipMemcpy(out.data(), t.slot(slot), t.slot_elems * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> h(t.slot_elems);
        HIP_TRY(hipMemcpy(h.data(), t.slot(slot), t.slot_elems * 2, hipMemcpyDeviceToHost));
        // activation tensors hold log2 e * a (irmv_common.hpp, "activation scale"); the network input does not
        const float unscale = t.name == "input" ? 1.0f : kActUnscale;
        for (size_t i = 0; i < t.slot_elems; i++) out[i] = half_bits_to_float(h[i]) * unscale;
    }
    return IRMV_OK;
}

// A step never writes the tensors inside a fused kernel ("input", "0", "model.2.cat", "model.2.tmp"): a read-back of one of
// them first runs the stand-alone layers the fused kernels cover, on the slot's current device frame.
static int materialize_fused(irmv_engine *e, int slot)
{
    if (e->lazy_tensors.empty()) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    TRY(enqueue_step(e, STEP_MATERIALIZE, slot, 1, e->stream, 1, nullptr));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->head_stale[slot] = 0;   // (the finals and the keypoint layers have written every head row)
    e->branch_stale[slot] = 0; // (... and the box branches' gated first convs their whole tensors)
    return IRMV_OK;
}

// The head of a slot whose last step stored candidate rows only (sparse_head): the read-back step runs the branches' finals
// and the keypoint layers as layers, which write every row -- the same bits the carriers compute.  A head written through
// irmv_engine_write_head since that step is not stale and stays as written.
static int ensure_dense_head(irmv_engine *e, int slot)
{
    if (!e->head_stale[slot]) return IRMV_OK;
    TRY(materialize_fused(e, slot));
    return IRMV_OK;
}

extern "C" int irmv_engine_read_input(irmv_engine *e, int slot, float *chw)
{
    TRY(check_range(e, slot, 1));
    TRY(materialize_fused(e, slot));
    std::vector<float> v;
    TRY(read_tensor_f32(e, e->tensors[e->tensor_idx.at("input")], slot, v));
    const size_t n = (size_t)e->cfg.net_size * e->cfg.net_height;
    for (size_t p = 0; p < n; p++)
        for (int c = 0; c < 3; c++) chw[c * n + p] = v[p * 4 + c];
    return IRMV_OK;
}

// the slot's head records as they lie in memory, in read_head's layout: [num_anchors][64 + nc + nk]
static int copy_head(irmv_engine *e, int slot, float *head)
{
    for (int l = 0; l < 3; l++) {
        std::vector<float> v;
        TRY(read_tensor_f32(e, e->tensors[e->head_t[l]], slot, v));
        for (int p = 0; p < e->lvl_hw[l]; p++) {
            float *o = head + (size_t)(e->lvl_base[l] + p) * e->no;
            const float *r = v.data() + (size_t)p * kHeadRec;
            memcpy(o, r, 64 * 4);
            memcpy(o + 64, r + kClsOff, (size_t)e->nc * 4);
            if (e->nk) memcpy(o + 64 + e->nc, r + kKptOff, (size_t)e->nk * 4);
        }
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_read_head(irmv_engine *e, int slot, float *head)
{
    TRY(check_range(e, slot, 1));
    TRY(ensure_dense_head(e, slot));
    return copy_head(e, slot, head);
}

// (tests) read_head without the read-back step in front: the rows as the last step or write_head left them -- after a sparse
// step only the candidate anchors' box and keypoint channels are that step's.  Runs no kernel and leaves head_stale alone.
extern "C" int irmv_engine_debug_read_head_raw(irmv_engine *e, int slot, float *head)
{
    TRY(check_range(e, slot, 1));
    if (!head) return fail(IRMV_ERR_ARG, "debug_read_head_raw: head is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    return copy_head(e, slot, head);
}

extern "C" int irmv_engine_write_head(irmv_engine *e, int slot, const float *head)
{
    TRY(check_range(e, slot, 1));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    for (int l = 0; l < 3; l++) {
        std::vector<float> v((size_t)e->lvl_hw[l] * kHeadRec, 0.f);
        for (int p = 0; p < e->lvl_hw[l]; p++) {
            const float *o = head + (size_t)(e->lvl_base[l] + p) * e->no;
            float *r = v.data() + (size_t)p * kHeadRec;
            memcpy(r, o, 64 * 4);
            memcpy(r + kClsOff, o + 64, (size_t)e->nc * 4);
            if (e->nk) memcpy(r + kKptOff, o + 64 + e->nc, (size_t)e->nk * 4);
        }
        HIP_TRY(hipMemcpy(e->tensors[e->head_t[l]].slot(slot), v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    e->head_stale[slot] = 0;
    return IRMV_OK;
}

extern "C" int irmv_engine_read_tap(irmv_engine *e, int slot, const char *name, float *nhwc, int shape[3])
{
    TRY(check_range(e, slot, 1));
    if (!name || !shape) return fail(IRMV_ERR_ARG, "name/shape is null");
    auto it = e->tensor_idx.find(name);
    if (it == e->tensor_idx.end()) return fail(IRMV_ERR_ARG, std::string("no tensor named ") + name);
    const Tensor &t = e->tensors[it->second];
    shape[0] = t.H; shape[1] = t.W; shape[2] = t.C;
    if (!nhwc) return IRMV_OK;
    // (a box branch's gated first conv is lazy only while its slot is stale: a read of it after the read-back step, or before any
    //  step, runs nothing and so leaves a head written through write_head alone)
    bool gated_out = false;
    for (const Op &op : e->ops) gated_out = gated_out || (op.gated_first && op.out_t == it->second);
    if (e->lazy_tensors.count(t.name) && (!gated_out || e->branch_stale[slot])) TRY(materialize_fused(e, slot));
    for (int l = 0; l < 3; l++) if (it->second == e->head_t[l]) TRY(ensure_dense_head(e, slot));
    std::vector<float> v;
    TRY(read_tensor_f32(e, t, slot, v));
    memcpy(nhwc, v.data(), v.size() * 4);
    return IRMV_OK;
}

// ---- per-layer conv test hooks (tests/test_gpu_conv_candidates.py) ---------------------
extern "C" int irmv_engine_read_tensor(irmv_engine *e, const char *name, int first, int count, void *dst, size_t bytes)
{
    TRY(check_range(e, first, count));
    if (!name) return fail(IRMV_ERR_ARG, "name is null");
    auto it = e->tensor_idx.find(name);
    if (it == e->tensor_idx.end()) return fail(IRMV_ERR_ARG, std::string("no tensor named ") + name);
    const Tensor &t = e->tensors[it->second];
    const size_t need = t.slot_elems * t.esize() * count;
    if (!dst || bytes != need) return fail(IRMV_ERR_ARG, "read_tensor: buffer size does not match the slot range");
    TRY(irmv_engine_wait(e));
    for (int l = 0; l < 3; l++)
        if (it->second == e->head_t[l]) for (int s = first; s < first + count; s++) TRY(ensure_dense_head(e, s));
    for (const Op &op : e->ops)   // a box branch's first conv behind the tile gate: stale outside the last step's active tiles
        if (op.gated_first && op.out_t == it->second)
            for (int s = first; s < first + count; s++) if (e->branch_stale[s]) TRY(materialize_fused(e, s));
    HIP_TRY(hipMemcpy(dst, t.slot(first), need, hipMemcpyDeviceToHost));
    return IRMV_OK;
}

extern "C" int irmv_engine_debug_read_head_rows(irmv_engine *e, int slot, float *rec, size_t bytes)
{
    TRY(check_range(e, slot, 1));
    if (!rec || bytes != (size_t)e->A * kHeadRec * sizeof(float)) return fail(IRMV_ERR_ARG, "debug_read_head_rows: the buffer must hold num_anchors x 96 floats");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    char *dst = reinterpret_cast<char *>(rec);
    for (int l = 0; l < 3; l++) {   // (no ensure_dense_head: the rows as the last step or write_head left them)
        const Tensor &t = e->tensors[e->head_t[l]];
        const size_t n = t.slot_elems * t.esize();
        HIP_TRY(hipMemcpy(dst, t.slot(slot), n, hipMemcpyDeviceToHost));
        dst += n;
    }
    return IRMV_OK;
}

static int conv_op_at(const irmv_engine *e, int op)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (op < 0 || op >= (int)e->ops.size() || e->ops[op].kind != OP_CONV) return fail(IRMV_ERR_ARG, "not a conv op");
    return IRMV_OK;
}

extern "C" int irmv_engine_conv_ops(irmv_engine *e, irmv_conv_op *ops, int cap, int *n)
{
    if (!e || !n) return fail(IRMV_ERR_ARG, "engine / n is null");
    auto name = [](char *dst, size_t cap_, const std::string &s) { snprintf(dst, cap_, "%s", s.c_str()); };
    auto seg = [&](irmv_conv_seg &d, const SegRef &s) {
        memset(&d, 0, sizeof d);
        if (s.t < 0 || s.C == 0) return;
        name(d.tensor, sizeof d.tensor, e->tensors[s.t].name);
        d.coff = s.coff; d.C = s.C; d.shift = s.shift;
    };
    int k = 0;
    for (size_t i = 0; i < e->ops.size(); i++) {
        const Op &op = e->ops[i];
        if (op.kind != OP_CONV) continue;
        if (ops && k < cap) {
            irmv_conv_op &r = ops[k];
            memset(&r, 0, sizeof r);
            r.op = (int32_t)i;
            name(r.layer, sizeof r.layer, op.layer);
            r.ks = op.cfg.ks; r.stride = op.cfg.stride; r.act = op.cfg.act; r.out_f32 = op.cfg.out_f32;
            r.cin = op.cin; r.cout = op.cout; r.cout_pad = op.cout_pad;
            r.Hin = op.Hin; r.Win = op.Win; r.Hout = op.Hout; r.Wout = op.Wout;
            seg(r.s0, op.s0);
            seg(r.s1, op.s1);
            if (op.res_t >= 0) seg(r.res, SegRef{op.res_t, op.res_coff, op.cout, 0});
            const Tensor &ot = e->tensors[op.out_t];
            name(r.out_tensor, sizeof r.out_tensor, ot.name);
            r.out_coff = op.out_coff;
            r.out_lazy = e->lazy_tensors.count(ot.name) ? 1 : 0;
            r.fused = op.fuse_next >= 0;
            r.tune_fused = op.tune_fuse[0] >= 0 || op.tune_fuse[1] >= 0;
            const int f = op.fuse_next >= 0 ? op.fuse_next : std::max(op.tune_fuse[0], op.tune_fuse[1]);
            if (f >= 0) {
                const Op &o2 = e->ops[f];
                name(r.fuse_layer, sizeof r.fuse_layer, o2.layer);
                name(r.fuse_tensor, sizeof r.fuse_tensor, e->tensors[o2.out_t].name);
                r.fuse_coff = o2.out_coff; r.fuse_cout = o2.cout; r.fuse_cout_pad = o2.cout_pad;
            }
            name(r.kname, sizeof r.kname, op.kname);
            name(r.kname_one, sizeof r.kname_one, op.kname_one);
        }
        k++;
    }
    *n = k;
    return IRMV_OK;
}

// The op as the tuner saw it at tune_count (which of its two passes, and the fused 1x1 that pass was tuned for);
// cands: that pass's candidate list, exactly as autotune_convs built it.
static int conv_tune_pass(const irmv_engine *e, int op, int tune_count, Op &o, std::vector<TuneCand> &cands)
{
    TRY(conv_op_at(e, op));
    const int share = stream_share(e, e->cfg.num_slots);
    if (tune_count != share && tune_count != 1) return fail(IRMV_ERR_ARG, "tune_count is neither the stream share nor 1");
    o = e->ops[op];
    o.fuse_next = o.tune_fuse[tune_count == share ? 0 : 1];
    const ConvView v = conv_view(e, o, 0, tune_count);
    cands = tune_candidates(o, v.a, tune_count, v.want_fuse, v.lds_ok, e->tune_sw, e->num_cus);
    return IRMV_OK;
}

extern "C" int irmv_engine_conv_candidates(irmv_engine *e, int op, int tune_count, irmv_conv_cand *out, int cap, int *n)
{
    if (!n) return fail(IRMV_ERR_ARG, "n is null");
    Op o;
    std::vector<TuneCand> cands;
    TRY(conv_tune_pass(e, op, tune_count, o, cands));
    for (size_t i = 0; i < cands.size() && out && (int)i < cap; i++) {
        irmv_conv_cand &r = out[i];
        memset(&r, 0, sizeof r);
        conv_cfg_name(cands[i].c, r.name, sizeof r.name);
        const TuneEntry t = tune_entry(cands[i].c);
        r.mt = t.mt; r.nt = t.nt; r.flags = t.flags; r.ipw = t.ipw;
        r.forced = cands[i].forced;
    }
    *n = (int)cands.size();
    return IRMV_OK;
}

extern "C" int irmv_engine_run_conv_candidate(irmv_engine *e, int op, int tune_count, int cand, int first, int count, uint32_t flags)
{
    TRY(check_range(e, first, count));
    Op o;
    std::vector<TuneCand> cands;
    TRY(conv_tune_pass(e, op, tune_count, o, cands));
    if (cand < -1 || cand >= (int)cands.size()) return fail(IRMV_ERR_ARG, "no such candidate");
    const Op &real = e->ops[op];
    // re-running a conv must not change its own inputs: refuse an output range that overlaps one of them
    auto overlaps = [](int t, int lo, int hi, int t2, int lo2, int hi2) { return t >= 0 && t == t2 && lo < hi2 && lo2 < hi; };
    const int o0 = real.out_coff, o1 = real.out_coff + real.cout_pad;
    if (overlaps(real.out_t, o0, o1, real.s0.t, real.s0.coff, real.s0.coff + real.s0.C) ||
        overlaps(real.out_t, o0, o1, real.s1.t, real.s1.coff, real.s1.coff + real.s1.C) ||
        overlaps(real.out_t, o0, o1, real.res_t, real.res_coff, real.res_coff + real.cout_pad))
        return fail(IRMV_ERR_ARG, "conv op writes one of its own inputs");
    TRY(irmv_engine_wait(e));
    ConvCfg c;
    if (cand >= 0) c = cands[cand].c;
    else {   // the engine's own choice for tune_count, with the epilogue a step runs it with
        o = real;
        c = tune_count == stream_share(e, e->cfg.num_slots) ? real.cfg : real.cfg_one;
    }
    const ConvView v = conv_view(e, o, first, count);
    if (flags & (IRMV_RUN_POISON | IRMV_RUN_POISON_ONLY)) {
        // all-ones bytes (a NaN in fp16 and in fp32) over the real output channels of the slots the run must write: the
        // fused 1x1's slice of the head when the run carries it (the 3x3's own output then never leaves the registers)
        const Op &w = v.a.n2 > 0 ? e->ops[o.fuse_next] : real;
        const Tensor &t = e->tensors[w.out_t];
        if (w.out_coff + w.cout > t.C) return fail(IRMV_ERR_ARG, "output channels out of range");
        HIP_TRY(hipMemset2DAsync(static_cast<char *>(t.slot(first)) + (size_t)w.out_coff * t.esize(), (size_t)t.C * t.esize(), 0xff,
                                 (size_t)w.cout * t.esize(), (size_t)count * t.H * t.W, e->stream));
        if (flags & IRMV_RUN_POISON_ONLY) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            return IRMV_OK;
        }
    }
    if (!run_conv(o, c, v.a, count, e->stream)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        return IRMV_DECLINED;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// ---- per-op test hooks (tests/test_gpu_graph_ops.py) ---------------------------------
static const char *op_kind_name(OpKind k)
{
    switch (k) {
    case OP_PRE: return "pre";
    case OP_CONV0: return "conv0";
    case OP_CONV: return "conv";
    case OP_POOL: return "pool";
    case OP_NMS: return "nms";
    case OP_LIGHT: return "light";
    case OP_FRONT: return "front";
    case OP_C2F2: return "c2f2";
    case OP_C2F32: return "c2f32";
    case OP_DW: return "dw";
    case OP_SHUF: return "shuffle";
    case OP_SCAN: return "scan";
    case OP_BNECK: return "bneck";
    case OP_KPT3: return "kpt3";
    case OP_DEMOSAIC: return "demosaic";
    case OP_CROP: return "crop";
    }
    return "?";
}

// The activation channels op writes: [*coff, *coff + *C) of tensor *t (-1: none).  The pool writes slices 1..3 of its
// tensor (slice 0 is its input); the ops that write a whole tensor (preprocess, model.0.conv, shuffle, fused kernels
// standing for a layer) record no channel count of their own.
static void op_output(const irmv_engine *e, const Op &op, int *t, int *coff, int *C)
{
    *t = op.out_t; *coff = 0; *C = 0;
    if (op.out_t < 0) return;
    const Tensor &ot = e->tensors[op.out_t];
    if (op.kind == OP_POOL) { *coff = ot.C / 4; *C = ot.C - ot.C / 4; return; }
    *coff = op.out_coff;
    *C = op.cout > 0 ? op.cout : ot.C - op.out_coff;
}

extern "C" int irmv_engine_ops(irmv_engine *e, irmv_graph_op *ops, int cap, int *n)
{
    if (!e || !n) return fail(IRMV_ERR_ARG, "engine / n is null");
    auto name = [](char *dst, size_t cap_, const std::string &s) { snprintf(dst, cap_, "%s", s.c_str()); };
    auto seg = [&](irmv_conv_seg &d, const SegRef &s) {
        memset(&d, 0, sizeof d);
        if (s.t < 0) return;
        name(d.tensor, sizeof d.tensor, e->tensors[s.t].name);
        d.coff = s.coff; d.C = s.C > 0 ? s.C : e->tensors[s.t].C - s.coff; d.shift = s.shift;
    };
    for (size_t i = 0; ops && i < e->ops.size() && (int)i < cap; i++) {
        const Op &op = e->ops[i];
        irmv_graph_op &r = ops[i];
        memset(&r, 0, sizeof r);
        r.op = (int32_t)i;
        name(r.kind, sizeof r.kind, op_kind_name(op.kind));
        name(r.layer, sizeof r.layer, op.layer);
        name(r.kname, sizeof r.kname, op.kname);
        seg(r.s0, op.kind == OP_POOL ? SegRef{op.out_t, 0, e->tensors[op.out_t].C / 4, 0} : op.s0);
        seg(r.s1, op.s1);
        int t, coff, C;
        op_output(e, op, &t, &coff, &C);
        if (t >= 0) {
            name(r.out_tensor, sizeof r.out_tensor, e->tensors[t].name);
            r.out_coff = coff; r.out_C = C;
        }
        r.fused_away = op.fused_away ? 1 : 0;
    }
    *n = (int)e->ops.size();
    return IRMV_OK;
}

extern "C" int irmv_engine_run_op(irmv_engine *e, int op, int first, int count, uint32_t flags)
{
    TRY(check_range(e, first, count));
    if (op < 0 || op >= (int)e->ops.size()) return fail(IRMV_ERR_ARG, "no such op");
    const Op &o = e->ops[op];
    if (o.kind != OP_CONV0 && o.kind != OP_POOL && o.kind != OP_DW && o.kind != OP_SHUF)
        return fail(IRMV_ERR_ARG, std::string("run_op runs conv0, pool, dw and shuffle ops, not ") + op_kind_name(o.kind));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    if (flags & (IRMV_RUN_POISON | IRMV_RUN_POISON_ONLY)) {   // all-ones bytes (an fp16 NaN) over what the run must write
        int t, coff, C;
        op_output(e, o, &t, &coff, &C);
        const Tensor &ot = e->tensors[t];
        if (coff + C > ot.C) return fail(IRMV_ERR_ARG, "output channels out of range");
        HIP_TRY(hipMemset2DAsync(static_cast<char *>(ot.slot(first)) + (size_t)coff * ot.esize(), (size_t)ot.C * ot.esize(), 0xff,
                                 (size_t)C * ot.esize(), (size_t)count * ot.H * ot.W, e->stream));
        if (flags & IRMV_RUN_POISON_ONLY) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            return IRMV_OK;
        }
    }
    launch_graph_op(e, o, first, count, e->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

extern "C" int irmv_sppf_slab(int batch, int H, int W, int C)
{
    if (batch < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0) return fail(IRMV_ERR_ARG, "sppf_slab: bad shape");
    return sppf_slab(batch, H, W, C);
}

extern "C" int irmv_engine_read_raw(irmv_engine *e, int slot, irmv_raw_dets *out)
{
    TRY(check_range(e, slot, 1));
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    const DevFrameOut &fo = e->fout_host[slot];
    const DevDet *d = e->dets_host + (size_t)slot * e->cfg.max_det;
    out->num_dets = fo.num_dets;
    out->n_candidates = fo.n_candidates;
    for (int i = 0; i < e->cfg.max_det; i++) {
        if (out->det_boxes) memcpy(out->det_boxes + 4 * i, d[i].box_net, 16);
        if (out->det_scores) out->det_scores[i] = d[i].score;
        if (out->det_classes) out->det_classes[i] = d[i].cls;
        if (out->det_anchors) out->det_anchors[i] = d[i].anchor;
        if (out->det_kpts) memcpy(out->det_kpts + 8 * i, d[i].kpts_net, 32);
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_profile(irmv_engine *e, int first, int count, irmv_kernel_stat *stats, int cap, int *n)
{
    TRY(check_range(e, first, count));
    if (!n) return fail(IRMV_ERR_ARG, "n is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    // Eager replay of the step's launches on the engine stream, every kernel bracketed by an event
    // pair.  The kernels are idempotent and are launched kProfileRepeat times inside their bracket: an event pair around ONE launch also times ~4 us of
    // command-processor hand-over, which would read as kernel time on these 5-80 us kernels.
    // (Event-record nodes inside a captured graph cannot be read back with hipEventElapsedTime on
    // ROCm 7.2: "invalid resource handle".)
    TRY(irmv_engine_wait(e));
    const StepKind kind = count == 1 ? STEP_ONE : STEP_BATCH;
    std::vector<EvRec> ev;   // (one per launch of the plan, in its order)
    TRY(enqueue_step(e, kind, first, count, e->stream, kProfileRepeat, &ev));   // (a window engine crops out of its device frames, as a submit without IRMV_SUBMIT_H2D does)
    if (e->window) std::copy(e->win_org.begin() + first, e->win_org.begin() + first + count, e->sub_org.begin() + first);
    if (e->sparse_head) std::fill(e->head_stale.begin() + first, e->head_stale.begin() + first + count, 1);
    if (e->sparse_branch) std::fill(e->branch_stale.begin() + first, e->branch_stale.begin() + first + count, 1);
    TRY(copy_out(e, first, count));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < ev.size(); i++) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i].a, ev[i].b));
        (void)hipEventDestroy(ev[i].a);
        (void)hipEventDestroy(ev[i].b);
        const Launch &l = e->plans[kind][i];
        if ((int)i < cap && stats) {
            irmv_kernel_stat &st = stats[i];
            memset(&st, 0, sizeof st);
            snprintf(st.name, sizeof st.name, "%s", l.name.c_str());
            snprintf(st.layer, sizeof st.layer, "%s", l.layer.c_str());
            st.flops = l.flops * count;
            st.bytes = l.bytes * count + l.launch_bytes;
            st.ms = l.once ? ms : ms / (float)kProfileRepeat;
        }
    }
    *n = (int)ev.size();
    return IRMV_OK;
}

// ---- PnPSolver -------------------------------------------------------------------------
struct irmv_pnp {
    int device = 0;
    PnpConst c{};
    hipStream_t stream = nullptr;
    float *pts = nullptr;
    double *rvec = nullptr, *tvec = nullptr;
    int32_t *ok = nullptr;
    int cap = 0;
};

static void pnp_free(irmv_pnp *p)
{
    if (p->pts) (void)hipFree(p->pts);
    if (p->rvec) (void)hipFree(p->rvec);
    if (p->tvec) (void)hipFree(p->tvec);
    if (p->ok) (void)hipFree(p->ok);
    p->pts = nullptr; p->rvec = p->tvec = nullptr; p->ok = nullptr; p->cap = 0;
}

extern "C" int irmv_pnp_create(int device, const double K[9], const double D[5], irmv_pnp **out)
{
    if (!K || !D || !out) return fail(IRMV_ERR_ARG, "null argument");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(IRMV_ERR_HIP, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<irmv_pnp> p(new irmv_pnp);
    p->device = device;
    p->c.fx = K[0]; p->c.fy = K[4]; p->c.cx = K[2]; p->c.cy = K[5];
    p->c.k1 = D[0]; p->c.k2 = D[1]; p->c.p1 = D[2]; p->c.p2 = D[3]; p->c.k3 = D[4];
    p->c.hy[0] = 135.0 / 2.0 / 1000.0; p->c.hy[1] = 225.0 / 2.0 / 1000.0;
    p->c.hz[0] = p->c.hz[1] = 55.0 / 2.0 / 1000.0;
    HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    *out = p.release();
    return IRMV_OK;
}

extern "C" void irmv_pnp_destroy(irmv_pnp *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    pnp_free(p);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

extern "C" int irmv_pnp_solve(irmv_pnp *p, const float *img_pts, int n, int armor_size, double *rvec, double *tvec, int32_t *ok)
{
    if (!p || !img_pts || !rvec || !tvec || !ok || n < 0) return fail(IRMV_ERR_ARG, "null argument");
    if (armor_size != IRMV_ARMOR_SMALL && armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (n > p->cap) {
        pnp_free(p);
        const int cap = std::max(n, 64);
        HIP_TRY(hipMalloc((void **)&p->pts, (size_t)cap * 32));
        HIP_TRY(hipMalloc((void **)&p->rvec, (size_t)cap * 24));
        HIP_TRY(hipMalloc((void **)&p->tvec, (size_t)cap * 24));
        HIP_TRY(hipMalloc((void **)&p->ok, (size_t)cap * 4));
        p->cap = cap;
    }
    HIP_TRY(hipMemcpyAsync(p->pts, img_pts, (size_t)n * 32, hipMemcpyHostToDevice, p->stream));
    launch_pnp_only(p->c, p->pts, n, armor_size, p->rvec, p->tvec, p->ok, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rvec, p->rvec, (size_t)n * 24, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(tvec, p->tvec, (size_t)n * 24, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(ok, p->ok, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return IRMV_OK;
}
