// Private to the engine's host files (engine*.cpp); include/ never sees it.  What every part needs -- the error helpers, the
// engine object and its pieces, the environment switches -- and the functions that cross the files' boundaries:
//   engine.cpp        error / version / device ABI, configuration and front geometry, create / destroy / getters, NUMA and
//                     window ABI, extract-parameter and Bayer-ISP setters, the PnP object
//   engine_graph.cpp  .irmw blob, tensors, weight packing, the op list (build_engine)
//   engine_tune.cpp   everything decided by timing at creation: conv tiles and their cache, head groups, the synchronous launch form
//   engine_plan.cpp   head fusion, the sparse head's reordering, the launch list of each step kind, the ops a feature appends
//                     to the steps and where their launches stand (append_op)
//   engine_step.cpp   kernel arguments, the per-op launcher, steps (Step), the upload decision (choose_upload / enqueue_upload),
//                     the record channels (Records<T>: pinning, where a step writes, result copies, delivery), graph capture,
//                     the one submit path of ordinary and tiled steps (submit_group), wait / results
//   engine_tiles.cpp  tiled search: its checks, the merge's device state and arguments, the tiled submit's call of submit_group,
//                     the merge hook, the merged results and the merge parameters
//   engine_hooks.cpp  read-backs, debug images, debug_*, LDS fill / probe, conv and op test hooks, the profiler, the light trace
//   engine_meter.cpp  frame metering: its checks and map, the record's host helpers, the on-demand call, the step's launch
//   engine_yaw.cpp    constrained pose: its checks, the two tables and who rewrites them, the step's launch, the stand-alone call
//   engine_posecov.cpp pose uncertainty: its checks, the option table, the step's launch, the stand-alone call
//   engine_track.cpp  armor tracks: the checks, the switch, stamps and camera poses, the launch behind a step, the stand-alone tracker
//   engine_patch.cpp  plate patches: their checks, the option table, the step's launch, the on-demand call
//   engine_number.cpp plate numbers: the model's checks, its .irmn file and upload, the switch, the step's launch, the on-demand call
#pragma once
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

namespace irmv { int fail(int code, const std::string &msg); }   // sets the calling thread's irmv_last_error text; returns code
#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(IRMV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

#define TRY(x)            \
    do {                  \
        int _rc = (x);    \
        if (_rc) return _rc; \
    } while (0)

struct LayerW {
    std::string name;
    int cin, cout, k, stride, act;
    int groups;         // > 1: depthwise (groups == cout, cin == 1)
    const uint16_t *w;  // OHWI fp16 bits (points into the blob copy)
    const float *b;
};

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

// Every device allocation of an engine says what a step may rely on in it ("device memory a step may rely on");
// dev_alloc takes the tag as a required argument, and irmv_engine_debug_fill_mem chooses the residue by it.
//   MEM_CONST    the host uploads it, no step writes it
//   MEM_ACT      an activation tensor (or the head): a step writes the channels its ops declare, pad channels stay +0
//   MEM_CARRIED  a step relies on what the last one left: a documented step-boundary invariant
//   MEM_SCRATCH  a step writes every word before it reads it
// The kind is how the words are used.  MEM_INDEX: some kernel uses a word as an index, count, offset or label; index_max is
// the largest value valid in every such use (a fill never puts anything else there).  The others are plain data by width.
enum MemClass { MEM_CONST = IRMV_MEM_CONST, MEM_ACT = IRMV_MEM_ACT, MEM_CARRIED = IRMV_MEM_CARRIED, MEM_SCRATCH = IRMV_MEM_SCRATCH };
enum MemKind { MEM_U8 = IRMV_MEM_U8, MEM_F16 = IRMV_MEM_F16, MEM_F32 = IRMV_MEM_F32, MEM_F64 = IRMV_MEM_F64, MEM_INDEX = IRMV_MEM_INDEX };
struct MemTag { MemClass cls; MemKind kind; uint32_t index_max; };
constexpr MemTag mem_const(MemKind k) { return {MEM_CONST, k, 0u}; }
constexpr MemTag mem_act(MemKind k) { return {MEM_ACT, k, 0u}; }
constexpr MemTag mem_scratch(MemKind k) { return {MEM_SCRATCH, k, 0u}; }
constexpr MemTag mem_scratch_index(uint32_t max) { return {MEM_SCRATCH, MEM_INDEX, max}; }
constexpr MemTag mem_carried_index(uint32_t max) { return {MEM_CARRIED, MEM_INDEX, max}; }
struct DevRange { std::string name; MemTag tag; void *base; size_t bytes; };

// The front's switches (front_plan): IRMV_FRONT_FASTX / _DIRECT / _TILE8 =0 clear them (the last keeps the 4-row tile); all
// on for the plan irmv_front_plan exports.
struct FrontSwitches { bool fastx = true, direct = true, tall = true; };

// The tuner's switches: autotune_convs reads them, and the conv test hooks list the same candidates from them.
struct TuneSwitches {
    bool untuned, verbose, warn;        // IRMV_AUTOTUNE=0, IRMV_AUTOTUNE_VERBOSE, IRMV_TUNE_WARN
    bool has_s2, has_wres;              // IRMV_FORCE_S2=lds|ct|deep, IRMV_FORCE_WRES=<n> (parity tests) are set ...
    std::string force_s2, force_wres;   // ... to these values (copies: an engine's hooks read them after the environment may have changed)
    bool force_pw, force_pwn, force_cm, force_w8, force_nt8, force_pf4;
    bool no_pw, no_pwn, no_pf2, no_pf4, no_cm, no_w8, no_nt8, no_wres, no_deep;
};

// Every IRMV_* environment switch the engine reads, read once at the top of irmv_engine_create (engine.cpp read_switches):
// each takes effect for every engine created after it is set.  (IRMV_LOG_ALLOC and IRMV_TUNE_CACHE are per process, not per
// engine, and are not here.)
struct EngineSwitches {
    TuneSwitches tune{};
    FrontSwitches front;
    bool fused_front = true, fused_c2f = true;   // IRMV_FUSED_FRONT=0: preprocess, model.0.conv and model.1.conv run as layers; IRMV_FUSED_C2F=0: no fused C2f kernel (model.2's, the 32-channel blocks')
    bool bneck64 = true;           // single-frame steps run the 64-channel Bottlenecks of the C2f blocks (and their cv2) as one launch each (IRMV_BNECK64=0: off)
    bool kpt3 = true;              // the keypoint branch of a Detect level as one launch (engines that do not merge the first-stage Detect convs; IRMV_KPT3=0: off)
    bool fused_head = true;        // IRMV_FUSED_HEAD=0: no Detect final 1x1 rides in the epilogue of the conv in front of it
    int merge_head0 = -1;          // IRMV_MERGE_HEAD0=0: never merge the first-stage Detect convs of a level, =1: always; else: engines that never batch
    bool group_head = true;        // IRMV_GROUP_HEAD=0: no grouped Detect-branch launches
    bool group_verbose = false;    // IRMV_GROUP_VERBOSE: the head groups' timings on stderr
    bool group_force = false;      // IRMV_GROUP_FORCE=1 (parity test): group even where the one launch timed slower
    bool has_streams = false; int streams = 0;   // IRMV_STREAMS=<n> is set, to this number of compute streams
    bool numa = true;              // IRMV_NUMA=0: plain hipHostMallocDefault wherever the creating thread happens to run
    bool inline_copies = false;    // IRMV_INLINE_COPIES=1: round-1 behaviour, copies on the compute stream
    bool graph_upload = true;      // uploads that ride the compute stream are a node of the step's graph (IRMV_GRAPH_UPLOAD=0: a separate launch in front of it; measured
                                   // again in round 5 with the upload kernel: 0.3365 - 0.3438 ms against 0.335 - 0.336 as the first node: no hiding of the graph's launch cost)
    int upload_kernel_blocks = 256;   // 0: synchronous single-frame uploads ride the copy engine like every other upload (IRMV_UPLOAD_KERNEL=0)
    bool window_upload = true;     // synchronous steps of one or two slots crop straight out of the pinned slot (IRMV_WINDOW_UPLOAD=0: upload, then crop)
    int sync_launch = -1;          // IRMV_SYNC_LAUNCH=graph|eager forces detect()'s launch form (0 | 1); anything else, e.g. "auto": choose_sync_launch times it
    bool split_scan = true;        // scan + box decode as a multi-workgroup kernel in front of nms_pnp (IRMV_SPLIT_SCAN=0: inside it)
    bool emit_scan = true, sparse_head = true, sparse_branch = true;   // IRMV_EMIT_SCAN=0: the class-branch conv epilogues emit no candidates; IRMV_SPARSE_HEAD=0: every head row is stored;
                                   // IRMV_SPARSE_BRANCH=0: no tile gate behind the class carriers
    bool sparse_gather = true;     // IRMV_SPARSE_GATHER=0: the box branch stays the tile-gated layer launches (no OP_BOXG launch in a step)
    bool gather_kpt = true;        // a gather launch computes its level's keypoint branch too and the step drops the OP_KPT3 launch (IRMV_GATHER_KPT=0: off)
    bool kpt3_named = false;       // IRMV_KPT3=1 set explicitly asks for kpt3_kernel by name: its launches stay (the rule IRMV_FORCE_WRES has)
    int gather_grid = 0;           // IRMV_SPARSE_GATHER_GRID=<n> (tests): workgroups of a box_gather launch; 0: one per CU
    bool zero_copy_results = true; // IRMV_ZERO_COPY_RESULTS=0: device records + a D2H copy in keypoint mode too
    bool post_keys_only = false;   // IRMV_POST_KEYS_ONLY=1 (tests): run_post's NMS ignores scan_decode_kernel's boxes and decodes its own, as a whole step's does
    bool nms_classwalk = true;     // IRMV_NMS_CLASSWALK=0
    int nms_prefilter = 1;         // PostArgs::prefilter.  IRMV_NMS_PREFILTER=0: crowded frames sort and mask every candidate (round-3 behaviour; bit-identical);
                                   // IRMV_NMS_PRE=<hi>,<lo> (experiment: size of the head of the list): hi | lo << 16
    bool meter_merge = true;       // frame_meter_kernel adds a lane-group of equal pixels once with its sample count (IRMV_METER_MERGE=0: one LDS add per sample; same bits)
    bool nms_stamps = false; int nms_stamps_slots = 0;   // IRMV_NMS_STAMPS=<n>: the NMS kernel stamps its phases, the destructor prints the first n slots' (at least four)
};

enum OpKind { OP_PRE, OP_CONV0, OP_CONV, OP_POOL, OP_NMS, OP_LIGHT, OP_FRONT, OP_C2F2, OP_C2F32, OP_DW, OP_SHUF, OP_SCAN, OP_BNECK, OP_KPT3, OP_BOXG, OP_DEMOSAIC, OP_CROP, OP_METER, OP_YAW, OP_PATCH, OP_NUMBER, OP_POSECOV };

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
    int boxg = -1;             // a box-branch conv: index of the OP_BOXG launch (k_boxg.hip) that computes its level's branch at the candidate anchors in the steps that
                               // gather (box_gathers); OP_BOXG itself: 1
    bool gated_first = false;  // a Detect box branch's first conv that some step runs behind the tile gate (sparse branch) or not at all (OP_BOXG): its tensor is lazy, the read-back step runs it densely
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
    bool cand_list = false;   // OP_BOXG: the plan's first -- cand_list_kernel runs in front of it, for every level's launch
    int kpt = -1;             // OP_BOXG: the level's OP_KPT3 op whose branch the launch computes too (the plan has dropped that launch); -1: box only
    int grid = 0;             // OP_BOXG: workgroups of the launch (irmv_engine_run_op's IRMV_RUN_GRID); 0: the engine's (IRMV_SPARSE_GATHER_GRID, else one per CU)
    bool once = false;        // not repeated under irmv_engine_profile (appends to, consumes or rewrites per-frame lists)
    std::string name, layer;  // irmv_engine_profile's row
    double flops = 0, bytes = 0, launch_bytes = 0;   // per frame; launch_bytes (the weights): once per launch
};

// What a step is: the plan of `kind` on slots [first, first + count).  Everything that follows from these fields is a member
// here, so launch_op, enqueue_step and get_graph take a Step and nothing beside it describes the step.
struct Step {
    StepKind kind;
    int first, count;
    int tile_frame = -1;        // >= 0: a tiled step (irmv_engine_submit_tiles): every slot crops its window out of this slot's frame, and the merge (k_tiles.hip) is its last node
    bool crop_pinned = false;   // OP_CROP reads the window out of the pinned slots: nothing was uploaded (UP_PINNED_CROP)
    bool tiled() const { return tile_frame >= 0; }
    // a tiled step's NMS writes DEVICE records also where the engine's ordinary steps write pinned host memory: the merge kernel
    // behind it reads them, and a D2H copy brings them to the host
    bool dev_records() const { return tiled(); }
    // the demosaic of a tiled step runs ONCE, on tile_frame's raw frame
    int bayer_first() const { return tiled() ? tile_frame : first; }
    int bayer_count() const { return tiled() ? 1 : count; }
    bool operator<(const Step &o) const { return std::tie(first, count, kind, tile_frame, crop_pinned) < std::tie(o.first, o.count, o.kind, o.tile_frame, o.crop_pinned); }
};

// A captured step: the step, and the two facts that belong to a graph only.
struct GraphKey {
    Step step;
    bool upload;   // the frames' upload is the graph's first node (UP_PINNED_CROP: there is none, and nothing in front of the graph either)
    int view;      // IRMV_VIEW_*: the view its slots were in when it was captured
    bool operator<(const GraphKey &o) const { return std::tie(upload, view, step) < std::tie(o.upload, o.view, o.step); }
};

// The form a submit's frame upload takes, decided in one place (choose_upload) and enqueued in one (enqueue_upload).
enum UploadForm {
    UP_NONE,          // no upload was asked for (a submit without IRMV_SUBMIT_H2D: the frames are on the device)
    UP_PINNED_CROP,   // nothing: the step's crop reads the window out of the pinned slots, so only the window crosses PCIe
    UP_KERNEL,        // whole frames, by k_pre.hip upload_frame_kernel
    UP_COPY,          // whole frames, one copy
    UP_BANDS,         // per slot the band of full-width rows its window covers
};
struct Upload { UploadForm form = UP_NONE; int first = 0, count = 0; };   // slots [first, first + count): a tiled step's frame_slot alone

// What a step sees in front of model.1's output -- the source frame and everything that follows from its size.  views[0]
// (IRMV_VIEW_WINDOW) is what e->cfg describes: the whole frame of an engine without a window, the window of one with it.
// views[1] (IRMV_VIEW_FRAME) exists on window engines only, from the first irmv_engine_set_view(.., IRMV_VIEW_FRAME) on: the
// full frame, read where the uploads or the demosaic put it, with no crop in front.
struct View {
    bool built = false;
    bool crop = false;                 // a step cuts the slot's window out of its full frame first (OP_CROP)
    int src_w = 0, src_h = 0;          // the source frame the front, the light extraction and the rotated image see
    uint8_t *frames = nullptr;         // [S][frame_bytes]: src_dev, or full_dev for the frame view
    size_t frame_bytes = 0;            // one such HWC frame (and the slot stride)
    AxisTap *tap_x = nullptr, *tap_y = nullptr;
    bool fused_front = false;          // OP_FRONT replaces preprocess + model.0.conv + model.1.conv in a step
    irmv_front_plan_t front{};         // the front's geometry as front_plan decided it: tile grid, stage bytes, box = the valid (non-padding) net-input column / row ranges,
                                       // fastx / fx_i0 / fx_step: every x tap is (i0 + 2 k, i0 + 2 k + 1; 1/2): the front kernel's 2 : 1 column path
    float scale_x = 1.f, scale_y = 1.f, off_x = 0.f, off_y = 0.f;   // PostArgs: net-input pixels -> this source frame
    signed char *light_labels = nullptr;   // label pool of the light extraction: light_pool bytes per slot
    size_t light_pool = 0;
    uint8_t *rot_dev = nullptr;        // [frame_bytes] irmv_engine_rotated_image
    std::vector<Launch> plans[STEP_POST + 1];   // per StepKind: the launches of such a step, in order (build_step_plans)
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

// The PnP object (engine.cpp; engine_yaw.cpp's stand-alone call)
struct irmv_pnp {
    int device = 0;
    PnpConst c{};
    hipStream_t stream = nullptr;
    float *pts = nullptr;
    double *rvec = nullptr, *tvec = nullptr;   // [cap][2][3]: irmv_pnp_solve uses the first half
    double *err = nullptr;                     // [cap][2]
    int32_t *ok = nullptr;
    DevYaw *yaw = nullptr;                     // [cap]: irmv_pnp_solve_yaw's records
    int cap = 0;
    double *cov_poses = nullptr;               // [cap][6]: irmv_pnp_pose_cov's poses (rvec, tvec) ...
    DevPoseCov *cov = nullptr;                 // [cap]: ... and its records
};
int pnp_reserve(irmv_pnp *p, int n);           // engine.cpp: the object's buffers for n quads

// A record channel: the records a step writes per slot -- its result list, or a feature's side records beside it -- and their
// way to the host.  `dev` is a dev_alloc range of the feature's own site (which says who writes and who reads it); pin() gives
// it the twin `host` in mapped, coherent pinned memory and that memory's device view `host_dev`.  A step writes ONE of the two
// -- step_at() decides which, and nothing else does --, copy() moves slots between them, the host reads `host` alone.
// per_slot: max_det, or 1 for a per-frame record.  One implementation for every channel (engine_step.cpp).
struct irmv_engine;
template <typename T> struct Records {
    T *dev = nullptr, *host = nullptr, *host_dev = nullptr;
    int per_slot = 0;
    T *dev_at(int slot) const { return dev + (size_t)slot * per_slot; }
    const T *host_at(int slot) const { return host + (size_t)slot * per_slot; }
    // the pinned twin of dev's first slots * per_slot records, both zeroed; `what`: log_range's text
    int pin(const irmv_engine *e, int slots, int per_slot, const char *what);
    // where step s writes its first slot's records: the pinned memory (zero-copy results) or the device records
    T *step_at(const irmv_engine *e, const Step &s) const;
    // slots [first, first + count) from one copy to the other on stream st
    int copy(int first, int count, hipMemcpyKind dir, hipStream_t st) const;
    int zero(int slots) const;   // both copies
    // the first min(num_dets, max_det, cap) records of the slot's pinned list -> out, their number -> *n
    int deliver(const irmv_engine *e, int slot, void *out, int cap, int *n) const;
    void free_host();
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
    bool emit_scan = false;   // candidates are emitted by the class-branch conv epilogues (needs split_scan's counters and all three levels fused)
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
    // Candidate lists of the OP_BOXG launches (k_boxg.hip): per level and slot the candidate pixels cand_list_kernel found in
    // the bitmap, and their number.  Scratch: a step writes every count, and every entry below it, before a gather launch reads.
    int *boxg_list = nullptr;    // level l, slot s: lvl_base[l] * S + s * lvl_hw[l] + [0, lvl_hw[l])
    int *boxg_count = nullptr;   // [3][S]
    int lvl_hw[3] = {0, 0, 0}, lvl_base[3] = {0, 0, 0};
    size_t frame_bytes = 0;       // one HWC source frame of src_dev (views[0])
    size_t src_bytes = 0;         // one source slot as the producer writes it (src_host, and raw_dev or src_dev): frame_bytes, or W*H for a Bayer engine
    hipStream_t stream = nullptr;                 // stream 0: single-slot detect(), read-backs, profile
    hipStream_t extra_streams[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // streams 1..num_streams-1
    int num_streams = 1;
    // frame hand-off: uploads can ride a stream of their own, chained to the compute streams by the
    // events of the submitted slot group
    hipStream_t h2d_stream = nullptr;
    std::map<std::pair<int, int>, SlotGroup> groups;   // (first, count) -> events of that group's last submit
    std::vector<SlotGroup *> slot_owner;               // per slot: the group whose submit touched it last
    uint8_t *src_host = nullptr;  // pinned [S][frame]
    int sync_launch = 0;               // how a synchronous single-frame step (detect()) reaches the GPU: 0 = one hipGraph replay (upload = its first node), 1 = launched
                                       // kernel by kernel behind the upload; chosen by timing at creation (choose_sync_launch), IRMV_SYNC_LAUNCH=graph|eager forces
    uint8_t *src_host_dev = nullptr;   // the same memory through the device's mapping (the upload kernel reads it: launch_upload_frames)
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
    // Search view (irmv_engine_set_view): per slot, whether its next step runs on its window or on the whole frame.
    View views[2];                    // [IRMV_VIEW_WINDOW], [IRMV_VIEW_FRAME]
    std::vector<int> slot_view;       // [S] IRMV_VIEW_* of the slot's next submit (all IRMV_VIEW_WINDOW = 0 until set_view)
    std::vector<int> sub_view;        // [S] ... as it was at the slot's last submit: whether its results carry the corner
    int front_ops[3] = {-1, -1, -1};  // ops preprocess, model.0.conv, model.1.conv: what a view whose front is not fused launches
    int front_op = -1;                // OP_FRONT: what a view whose front is fused launches in their place (-1: no view's is)
    // Tiled search (irmv_engine_submit_tiles / irmv_engine_merge_tiles): nothing below exists until the first tiled call.
    // tile_params_dev: the two floats the merge kernel reads when it runs (irmv_engine_set_tile_merge rewrites them, graphs hold
    // the address).  tile_merges[first]: the merged list of the last tiled step or merge whose first slot was `first` -- device
    // record, pinned copy, and whether one has run.
    struct TileMerge { TileOut *out_dev = nullptr, *out_host = nullptr; int count = 0; bool valid = false; };
    TileMergeParams *tile_params_dev = nullptr;
    TileMergeParams tile_params{0.5f, 2.0f};
    std::map<int, TileMerge> tile_merges;
    PnpConst pnp_base{};              // the camera as configured; pnp_dev[slot] = pnp_base with the principal point moved by the slot's corner
    std::vector<Tensor> tensors;
    std::map<std::string, int> tensor_idx;
    std::vector<Op> ops;
    std::vector<DevRange> dev_allocs;     // every device range of the engine, classified (dev_alloc)
    int head_t[3] = {-1, -1, -1};
    float *head_all = nullptr;
    PnpConst *pnp_dev = nullptr;
    // Class policy (irmv_engine_set_class_policy): cls_dev[0] is the table every threshold site and plate pick reads, cls_dev[1]
    // its mute twin -- all thresholds +inf, the same plates -- behind the muted repetitions of irmv_engine_profile.  The
    // addresses are fixed for the engine's life; a policy change rewrites the contents and re-captures nothing.
    ClassTable *cls_dev = nullptr;
    irmv_class_policy policy{};       // the policy in force (the uniform one of cfg.score_thr / cfg.armor_size until set)
    // Pose ambiguity (irmv_engine_set_pose_prior).  Until the first call nothing but `up` and `pose_prior` (host values) exists
    // and every step launches what it always has.  The first call allocates the alt records (`alts` below), the prior table and
    // the per-slot up vectors, and drops the captured graphs once: from then on the steps launch the kAlt kernels, which read
    // both tables when they run.
    bool pose_alt = false;
    PosePrior *prior_dev = nullptr;
    double *up_dev = nullptr;             // [S][3]
    std::vector<double> up;               // [S][3] unit vectors as set (default (0, -1, 0)), in the frame PnP sees
    irmv_pose_prior pose_prior{};         // the prior in force (MIN_ERR, ratio 8, every normal_up 0 until set)
    long long *dbg_dev = nullptr;
    std::set<std::string> lazy_tensors;   // tensors a step does not write because a fused kernel keeps them on chip
    bool classical = false;            // four points from the classical light extraction instead of a keypoint head
    // Refined point source (IRMV_POINTS_REFINED): the keypoint engine's step plus the guided light extraction behind the NMS
    // (k_light.hip, light_extract_kernel<true>).  `classical` stays false: the keypoint decode runs.  A refined engine has the
    // classical engine's per-slot scratch and device records; refine_dev (the two live floats the kernel reads when it runs;
    // graphs hold the address) and refine_kpts (the prior, [S][max_det][8]) exist from creation.  On any other engine both are
    // made by the first irmv_engine_refine_points ([max_det][8]) and nothing else changes.
    bool refined = false;
    RefineParams refine{0.5f, 4.0f};
    RefineParams *refine_dev = nullptr;
    float *refine_kpts = nullptr;
    short *light_points = nullptr, *light_hulls = nullptr;
    float *light_boxes = nullptr;      // explicit boxes of irmv_engine_extract_armors
    DevDet *light_dets_dev = nullptr, *light_dets_host = nullptr;
    LightTrace *light_trace_dev = nullptr;   // [max_det], allocated by the first irmv_engine_light_trace
    // Debug images (irmv_engine_render): nothing below exists until the first call.  render_out holds the largest picture any
    // view of the engine gives (scale 1); render_marks_host is what the mark upload reads (it outlives the call).
    RenderMark *render_marks = nullptr;      // [max_det]
    RenderFont *render_font = nullptr;
    uint8_t *render_out = nullptr;
    std::vector<RenderMark> render_marks_host;
    // Frame metering (irmv_engine_meter / irmv_engine_set_metering): nothing below exists until the first metering call.  That
    // call makes the scratch: the partials slab, the two parameter records -- [0] the step's, [1] the on-demand call's -- and the
    // device records (`meter` below), [num_slots] the steps' and one more for the on-demand call.  The first set_metering with
    // options pins the steps' records, appends the op (meter_op: its launch stands in every view's step plans) and drops the
    // captured graphs once.
    uint32_t *meter_slab = nullptr;          // [S][kMeterBlocksMax][4][256]
    MeterParams *meter_params_dev = nullptr; // [2]
    int meter_op = -1;                       // >= 0: the steps meter
    bool meter_on = false;                   // the options in force are not "off"
    irmv_meter_opts meter_opts{};
    float *boxes = nullptr;
    unsigned long long *keys = nullptr;
    // The record channels, in copy-out order.  dets and fout exist from creation; each of the others from its feature's first
    // enable (the comments above), with [S][max_det] records -- meter: [S + 1] device records, of which the first S are pinned.
    Records<MeterStats> meter;
    Records<DevDet> dets;
    Records<DevFrameOut> fout;
    Records<DevAlt> alts;
    Records<DevYaw> yaw;
    Records<DevPoseCov> posecov;
    Records<DevPatch> patch;
    Records<DevNumber> number;
    Records<DevDetTrack> dettrack;
    Records<DevTrackSnap> tracks;
    bool zero_copy_results = false;   // the NMS kernel writes its results straight into pinned host memory (no D2H copy)
    half_t *conv0_w = nullptr;
    float *conv0_b = nullptr;
    PostArgs post{};                  // (scale and offset: filled per step from the slots' view)
    std::map<GraphKey, hipGraphExec_t> graphs;
    double last_detect_ms = 0;
    std::vector<uint8_t> blob;
    std::vector<LayerW> layers;
    std::vector<std::vector<uint16_t>> dequant;   // int8 blobs: per layer fp16(q * scale), what LayerW::w points to
    std::vector<std::vector<uint16_t>> merged_w;  // Detect first-stage convs of a level concatenated along cout (single-frame engines)
    std::vector<std::vector<float>> merged_b;
    bool merge_head0 = false;
    EngineSwitches sw{};       // the environment as irmv_engine_create found it
    // Constrained pose (irmv_engine_set_yaw_solve): nothing below but yaw_opts (a host value) exists until the first call.  It
    // allocates the records (`yaw` above), the table and the per-slot bases, appends the op (yaw_op, behind the NMS / the light
    // extraction in every step plan and run_post's) and drops the captured graphs once.  set_up, set_pose_prior and later calls
    // rewrite the two tables (write_yaw_tables).
    int yaw_op = -1;
    irmv_yaw_opts yaw_opts{};
    YawTable *yaw_table_dev = nullptr;
    YawBasis *yaw_basis_dev = nullptr;        // [S]
    // Pose uncertainty (irmv_engine_set_pose_cov): nothing below but posecov_opts (a host value) exists until the first call.  It
    // allocates the records (`posecov` above) and the option table, appends the op (posecov_op: behind the yaw op's launch
    // where there is one, else behind the NMS / the light extraction) and drops the captured graphs once.  Later calls rewrite
    // the table.
    int posecov_op = -1;
    irmv_pose_cov_opts posecov_opts{};
    PoseCovTable *posecov_table_dev = nullptr;
    // Plate patches (irmv_engine_set_patches).  Nothing below but patch_opts (a host value) exists until the first set_patches
    // -- the records (`patch` above), the table, the op (patch_op, placed as yaw_op is), one drop of the captured graphs -- or
    // the first irmv_engine_patches_at: the table and the call's three buffers.
    int patch_op = -1;
    irmv_patch_opts patch_opts{};
    PatchTable *patch_table_dev = nullptr;
    float *patch_at_kpts = nullptr;           // [kMaxDetCap][8]
    int32_t *patch_at_sizes = nullptr;        // [kMaxDetCap]
    DevPatch *patch_at_out = nullptr;         // [kMaxDetCap]
    // Plate numbers (irmv_engine_set_number_model / irmv_engine_set_numbers).  Nothing below but number_opts (a host value)
    // exists until the first set_number_model: the table, the weights and the biases, each sized for the largest model, at
    // addresses that never move -- a later model rewrites their contents and re-captures nothing.  The first set_numbers makes
    // the records (`number` above) and the op (number_op, directly behind the patch op's launch) and drops the captured graphs
    // once; the first irmv_engine_numbers_at the call's two buffers.
    int number_op = -1;
    bool number_model = false;                // a model has been set
    irmv_number_opts number_opts{};
    NumberTable number_table{};               // the table as uploaded last (enable: number_opts.enable)
    NumberTable *number_table_dev = nullptr;
    half_t *number_weights = nullptr;         // [kNumWeightHalves]
    float *number_bias = nullptr;             // [kNumBiasFloats]
    DevPatch *number_at_in = nullptr;         // [kMaxDetCap]
    DevNumber *number_at_out = nullptr;       // [kMaxDetCap]
    // Armor tracks (irmv_engine_set_tracking).  Nothing below but track_opts and track_slots (host values) exists until the first
    // set_tracking: the two channels (`dettrack`, `tracks` above), the carried table, the option table, the per-slot stamps and
    // camera poses, the event.  There is no op and no graph node: track_step launches behind an ordinary step on the step's
    // stream and chains the launches of different streams by track_event, in submit order.
    bool track_made = false;
    irmv_track_opts track_opts{};
    std::vector<TrackSlot> track_slots;       // [S] stamp and camera pose as set (0, identity, 0)
    DevTrackTable *track_table_dev = nullptr;
    TrackOpts *track_opts_dev = nullptr;
    TrackSlot *track_slots_dev = nullptr;     // [S]
    hipEvent_t track_event = nullptr;         // recorded behind the last track launch ...
    hipStream_t track_event_stream = nullptr; // ... on this stream (nullptr: none since the last irmv_engine_wait of set_tracking)

    ~irmv_engine();
};

constexpr int kProfileRepeat = 4;   // launches per event bracket in irmv_engine_profile

struct TuneEntry { int mt, nt, flags, ipw; };   // a choice as the IRMV_TUNE_CACHE file holds it (flags: tile_flags)
// forced: an IRMV_FORCE_* switch puts the layer on this candidate (parity tests) -- the last forced one that runs is the choice
struct TuneCand { ConvCfg c; bool forced; };
// How the tuner sees a conv op on slots [first, first + count): its arguments, whether it is tuned for its branch's final
// 1x1 in the epilogue (op.fuse_next), and its kernel family.  autotune_convs and the conv test hooks both use it.
struct ConvView { ConvArgs a; bool want_fuse, lds_ok; };

// slots handled by one stream of a multi-slot submit
inline int stream_share(const irmv_engine *e, int count) { return (count + e->num_streams - 1) / e->num_streams; }
// the device memory an upload of the source slots writes: the raw slots of a Bayer engine, else the HWC frames themselves
// (a window engine's full frames)
inline uint8_t *upload_dev(const irmv_engine *e) { return e->raw_dev ? e->raw_dev : (e->window ? e->full_dev : e->src_dev); }
// the view slot's next step runs in
inline const View &view_of(const irmv_engine *e, int slot) { return e->views[e->slot_view[slot]]; }
// profile / op name of a Bayer engine's demosaic as it runs now
inline const char *demosaic_kname(const irmv_engine *e) { return e->bayer_mhc ? "bayer_demosaic_mhc" : (e->bayer_table ? "bayer_demosaic_lut" : "bayer_demosaic"); }
inline ConvWeights conv_weights(const Op &op) { return {op.w_packed, {op.w_lds[0], op.w_lds[1], op.w_lds[2], op.w_lds[3]}, op.w_k16}; }
inline bool run_conv(const Op &op, const ConvCfg &c, const ConvArgs &a, int count, hipStream_t s) { return launch_conv(c, a, conv_weights(op), count, s); }

namespace irmv {
// engine.cpp
void log_range(const irmv_engine *e, const char *what, const void *p, size_t bytes);
bool upload_aligned(size_t src_bytes, int first, int count);
void front_plan(const irmv_engine_cfg &c, const FrontSwitches &sw, irmv_front_plan_t *p, std::vector<AxisTap> &tx, std::vector<AxisTap> &ty);
int check_letterbox(const irmv_engine_cfg &c);
int write_window(irmv_engine *e, int slot);
int write_isp_table(irmv_engine *e);
int write_class_table(irmv_engine *e);
void drop_graphs(irmv_engine *e, bool keep_post);
int check_window_slot(const irmv_engine *e, int slot, const char *who);
int resolve_cfg(const irmv_engine_cfg *cfg_in, irmv_engine_cfg *full);
int window_map(int full_w, int full_h, int win_w, int win_h, int rotate180, const double K[9], int x0, int y0, irmv_window_map_t *m);
// engine_graph.cpp
int dev_alloc(irmv_engine *e, void **p, size_t bytes, const std::string &name, MemTag tag);
int load_blob(irmv_engine *e);
int build_engine(irmv_engine *e);
int build_view_geometry(irmv_engine *e, View &v, int src_w, int src_h);
int build_frame_view(irmv_engine *e);
// engine_tune.cpp
TuneEntry tune_entry(const ConvCfg &c);
std::vector<TuneCand> tune_candidates(const Op &op, const ConvArgs &a, int count, bool want_fuse, bool lds_ok, const TuneSwitches &sw, int num_cus);
ConvView conv_view(const irmv_engine *e, const Op &op, int first, int count);
int autotune_convs(irmv_engine *e);
int build_head_groups(irmv_engine *e);
int choose_sync_launch(irmv_engine *e);
// engine_plan.cpp
void finalize_head_fusion(irmv_engine *e);
void build_step_plans(irmv_engine *e, View &v);
void append_op(irmv_engine *e, OpKind kind);   // OP_METER, OP_YAW, OP_POSECOV, OP_PATCH or OP_NUMBER, at its feature's first enable
// engine_step.cpp
void fill_conv_args(const irmv_engine *e, const Op &op, int first, int count, ConvArgs &a, bool fused = false);
int slots_view(const irmv_engine *e, int first, int count, int *view = nullptr);
LightArgs light_args(const irmv_engine *e, const View &v, int first);
PostArgs post_args(const irmv_engine *e, const View &v, const Step &s);
bool launch_head_group(const irmv_engine *e, const irmv_engine::HeadGroup &g, int first, const PostArgs *pa, unsigned scan, hipStream_t s);
int launch_op(irmv_engine *e, const View &v, const Launch &l, const Step &s, const PostArgs &pa, unsigned scan, hipStream_t st);
int enqueue_step(irmv_engine *e, const Step &s, hipStream_t st, int reps = 1, const std::vector<hipEvent_t> *ev = nullptr);
void note_submit_windows(irmv_engine *e, int first, int count);
void mark_stepped(irmv_engine *e, int first, int count);
int copy_out(irmv_engine *e, int first, int count, hipStream_t st = nullptr);
MeterArgs meter_args(const irmv_engine *e, const View &v, int first, const MeterParams *params, MeterStats *out);
int check_range(const irmv_engine *e, int first, int count);
int load_frame(irmv_engine *e, int slot, hipStream_t st);
void det_pose(const DevDet &d, bool shift, float ox, float oy, irmv_det &o);
void slot_det(const irmv_engine *e, int slot, int i, irmv_det &o);
Upload choose_upload(const irmv_engine *e, int first, int count, int tile_frame, bool copy_engine, bool captured);
int enqueue_upload(irmv_engine *e, const Upload &u, hipStream_t st);
int get_graph(irmv_engine *e, const Step &s, const Upload &upload, hipGraphExec_t *out);
int submit_group(irmv_engine *e, int first, int count, uint32_t flags, hipStream_t st, int tile_frame = -1);
// engine_tiles.cpp
TileArgs tile_args(const irmv_engine *e, int first, int count);
// engine_hooks.cpp
int ensure_dense_head(irmv_engine *e, int slot);
// engine_yaw.cpp
void yaw_opts_defaults(irmv_yaw_opts *o);
int write_yaw_tables(irmv_engine *e, int slot = -1);   // no-op before the first set_yaw_solve; slot >= 0: that slot's basis alone
void launch_yaw(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st);
// engine_posecov.cpp
void pose_cov_opts_defaults(irmv_pose_cov_opts *o);
void launch_posecov(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st);
// engine_track.cpp
void track_opts_defaults(irmv_track_opts *o);
int track_step(irmv_engine *e, const Step &s, hipStream_t st);                 // behind an ordinary step: the table advances over its slots
int track_skip(irmv_engine *e, int first, int count, hipStream_t st, bool copied);   // a step that does not feed the tracker: its slots' channels read as zero
// engine_patch.cpp
void patch_opts_defaults(irmv_patch_opts *o);
void launch_patch(const irmv_engine *e, const View &v, const Step &s, const PostArgs &pa, hipStream_t st);
int enable_patches(irmv_engine *e);   // the first set_patches' part, for a caller that has waited for the engine
int write_patch_table(irmv_engine *e);
// engine_number.cpp
void launch_number(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st);
}
