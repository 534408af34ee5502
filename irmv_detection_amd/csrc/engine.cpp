// libirmv_hip.so host side: engine object, execution plan, hipGraph capture, C ABI.  This file: the object's life and its
// configuration; engine_internal.hpp says where the rest lives.
//
// MI355X-first counterpart of irmv_detection::YoloEngine (reference
// src/yolo_engine.cpp) and PnPSolver (src/pnp_solver.cpp):
//   * frame slots are pinned host memory (hipHostMalloc) copied to HBM by an
//     async copy on a dedicated upload stream, event-chained to the captured
//     step (results need no download: the NMS kernel stores its records straight into mapped pinned host memory;
//     only the classical and the refined point source keep device records + one D2H copy) -- the dGPU
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
#include "engine_internal.hpp"

static thread_local std::string g_err;
int irmv::fail(int code, const std::string &msg) { g_err = msg; return code; }

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

// Optional allocation log (IRMV_LOG_ALLOC=1): every device / pinned range an engine owns, so that a faulting
// address reported by the driver can be mapped to a buffer.
static bool log_alloc() { static const bool on = getenv("IRMV_LOG_ALLOC") != nullptr; return on; }
void irmv::log_range(const irmv_engine *e, const char *what, const void *p, size_t bytes)
{
    if (log_alloc()) fprintf(stderr, "[irmv alloc] engine %p %-18s [%p, %p) %zu bytes\n", (const void *)e, what, p, (const void *)((const char *)p + bytes), bytes);
}

// Destroy the engine's captured graphs -- their steps are captured again on next use --; keep_post: all but run_post's.
void irmv::drop_graphs(irmv_engine *e, bool keep_post)
{
    for (auto it = e->graphs.begin(); it != e->graphs.end();) {
        if (keep_post && it->first.step.kind == STEP_POST) { ++it; continue; }
        (void)hipGraphExecDestroy(it->second);
        it = e->graphs.erase(it);
    }
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
            for (int s = 0; s < cfg.num_slots && s < std::max(4, sw.nms_stamps_slots); s++)   // IRMV_NMS_STAMPS=<n> as it was when the engine was created: the first n slots (at least four)
            {
                const long long *t = &h[(size_t)s * 16];
                fprintf(stderr, "[nms stamps] slot %d: keys %lld select %lld decode %lld sort %lld gather+classes %lld rows %lld walk %lld kpts %lld pnp %lld store %lld cycles; total %lld; n=%lld kept=%lld\n", s,
                        t[7] - t[0], t[8] - t[7], t[9] - t[8], t[1] - t[9], t[10] - t[1], t[2] - t[10], t[3] - t[2], t[11] - t[3], t[12] - t[11], t[4] - t[12], t[4] - t[0], t[5], t[6]);
            }
    }
    drop_graphs(this, false);
    if (log_alloc()) fprintf(stderr, "[irmv alloc] engine %p destroy: freeing %zu device ranges\n", (const void *)this, dev_allocs.size());
    for (const DevRange &r : dev_allocs) (void)hipFree(r.base);
    dev_allocs.clear();
    if (src_host) (void)hipHostFree(src_host);
    dets.free_host(); fout.free_host(); alts.free_host(); yaw.free_host(); posecov.free_host(); dettrack.free_host(); tracks.free_host(); patch.free_host(); number.free_host(); meter.free_host();   // the record channels
    if (light_dets_host) (void)hipHostFree(light_dets_host);
    for (auto &kv : tile_merges)
        if (kv.second.out_host) (void)hipHostFree(kv.second.out_host);
    if (track_event) (void)hipEventDestroy(track_event);
    for (auto &kv : groups) {
        if (kv.second.h2d) (void)hipEventDestroy(kv.second.h2d);
        if (kv.second.out) (void)hipEventDestroy(kv.second.out);
    }
    for (int i = 0; i < 7; i++)
        if (extra_streams[i]) (void)hipStreamDestroy(extra_streams[i]);
    if (h2d_stream) (void)hipStreamDestroy(h2d_stream);
    if (stream) (void)hipStreamDestroy(stream);
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
bool irmv::upload_aligned(size_t src_bytes, int first, int count)
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
void irmv::front_plan(const irmv_engine_cfg &c, const FrontSwitches &sw, irmv_front_plan_t *p, std::vector<AxisTap> &tx, std::vector<AxisTap> &ty)
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

// The process's environment as one EngineSwitches.  Parsing per switch: `off` = the value starts with '0', `is1` = with '1',
// `set` = present with any value.
static EngineSwitches read_switches()
{
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto starts = [](const char *name, char c) { const char *v = getenv(name); return v && v[0] == c; };
    auto off = [&](const char *name) { return starts(name, '0'); };
    auto is1 = [&](const char *name) { return starts(name, '1'); };
    EngineSwitches s;
    TuneSwitches &t = s.tune;
    t.untuned = off("IRMV_AUTOTUNE"); t.verbose = set("IRMV_AUTOTUNE_VERBOSE"); t.warn = set("IRMV_TUNE_WARN");
    const char *s2 = getenv("IRMV_FORCE_S2"), *wres = getenv("IRMV_FORCE_WRES");
    t.has_s2 = s2 != nullptr; t.force_s2 = s2 ? s2 : "";
    t.has_wres = wres != nullptr; t.force_wres = wres ? wres : "";
    t.force_pw = set("IRMV_FORCE_PW"); t.force_pwn = set("IRMV_FORCE_PWN"); t.force_cm = set("IRMV_FORCE_CM");
    t.force_w8 = set("IRMV_FORCE_W8"); t.force_nt8 = set("IRMV_FORCE_NT8"); t.force_pf4 = set("IRMV_FORCE_PF4");
    t.no_pw = set("IRMV_NO_PW"); t.no_pwn = set("IRMV_NO_PWN"); t.no_pf2 = set("IRMV_NO_PF2"); t.no_pf4 = set("IRMV_NO_PF4");
    t.no_cm = set("IRMV_NO_CM"); t.no_w8 = set("IRMV_NO_W8"); t.no_nt8 = set("IRMV_NO_NT8"); t.no_wres = set("IRMV_NO_WRES");
    t.no_deep = is1("IRMV_NO_DEEP");
    s.front.fastx = !off("IRMV_FRONT_FASTX"); s.front.direct = !off("IRMV_FRONT_DIRECT"); s.front.tall = !off("IRMV_FRONT_TILE8");
    s.fused_front = !off("IRMV_FUSED_FRONT"); s.fused_c2f = !off("IRMV_FUSED_C2F"); s.bneck64 = !off("IRMV_BNECK64"); s.kpt3 = !off("IRMV_KPT3");
    s.fused_head = !off("IRMV_FUSED_HEAD");
    s.merge_head0 = off("IRMV_MERGE_HEAD0") ? 0 : (is1("IRMV_MERGE_HEAD0") ? 1 : -1);
    s.group_head = !off("IRMV_GROUP_HEAD"); s.group_verbose = set("IRMV_GROUP_VERBOSE"); s.group_force = set("IRMV_GROUP_FORCE");
    if (const char *ns = getenv("IRMV_STREAMS")) { s.has_streams = true; s.streams = atoi(ns); }
    s.numa = !off("IRMV_NUMA");
    s.inline_copies = is1("IRMV_INLINE_COPIES"); s.graph_upload = !off("IRMV_GRAPH_UPLOAD"); s.window_upload = !off("IRMV_WINDOW_UPLOAD");
    if (const char *uk = getenv("IRMV_UPLOAD_KERNEL")) s.upload_kernel_blocks = atoi(uk);
    s.sync_launch = starts("IRMV_SYNC_LAUNCH", 'e') ? 1 : (starts("IRMV_SYNC_LAUNCH", 'g') ? 0 : -1);
    s.split_scan = !off("IRMV_SPLIT_SCAN"); s.emit_scan = !off("IRMV_EMIT_SCAN");
    s.sparse_head = !off("IRMV_SPARSE_HEAD"); s.sparse_branch = !off("IRMV_SPARSE_BRANCH");
    s.sparse_gather = !off("IRMV_SPARSE_GATHER");
    s.gather_kpt = !off("IRMV_GATHER_KPT"); s.kpt3_named = is1("IRMV_KPT3");
    if (const char *gg = getenv("IRMV_SPARSE_GATHER_GRID")) s.gather_grid = atoi(gg);
    s.zero_copy_results = !off("IRMV_ZERO_COPY_RESULTS"); s.post_keys_only = is1("IRMV_POST_KEYS_ONLY");
    s.nms_classwalk = !off("IRMV_NMS_CLASSWALK");
    s.meter_merge = !off("IRMV_METER_MERGE");
    s.nms_prefilter = off("IRMV_NMS_PREFILTER") ? 0 : 1;
    if (const char *pe = getenv("IRMV_NMS_PRE")) { int hi = 0, lo = 0; if (sscanf(pe, "%d,%d", &hi, &lo) == 2 && hi >= 64 && hi <= 512 && lo >= 32 && lo < hi) s.nms_prefilter = hi | (lo << 16); }
    if (const char *st = getenv("IRMV_NMS_STAMPS")) { s.nms_stamps = true; s.nms_stamps_slots = atoi(st); }
    return s;
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

// a source so oblong that the short side of its letterboxed frame rounds to nothing: no box, no scale back to the source
int irmv::check_letterbox(const irmv_engine_cfg &c)
{
    int nw, nh;
    scaled_size(c, &nw, &nh);
    if (nw < 1 || nh < 1) return fail(IRMV_ERR_ARG, "letterbox: the scaled frame has no row or no column; use IRMV_RESIZE_STRETCH");
    return IRMV_OK;
}

// The caller's configuration at this library's size (an older caller's prefix, the appended fields at their defaults),
// and the checks of everything the front's geometry follows from.  No GPU call.
int irmv::resolve_cfg(const irmv_engine_cfg *cfg_in, irmv_engine_cfg *full)
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
    return check_letterbox(window_view(*cfg));
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

static int refined_needs_head() { return fail(IRMV_ERR_MODEL, "point_source = refined, but the model has no keypoint head"); }

// nk of the blob's header without a GPU call: -1 where only the device holds the blob; an unreadable or short blob is left
// to load_blob's own errors (-1 too).
static int peek_blob_nk(const irmv_engine_cfg &c, int *nk)
{
    uint8_t h[32] = {0};   // engine_graph.cpp BlobHeader
    *nk = -1;
    size_t got = 0;
    if (c.weights_path) {
        std::string path = c.weights_path;
        const size_t dot = path.find_last_of('.');
        if (dot != std::string::npos && path.substr(dot) != ".irmw") path = path.substr(0, dot) + ".irmw";
        std::ifstream f(path, std::ios::binary);
        if (f) { f.read(reinterpret_cast<char *>(h), sizeof h); got = (size_t)f.gcount(); }
    } else if (c.weights_blob && c.weights_bytes && !c.weights_on_device) {
        got = std::min<size_t>(sizeof h, c.weights_bytes);
        memcpy(h, c.weights_blob, got);
    }
    if (got == sizeof h && memcmp(h, "IRMW", 4) == 0) {   // char magic[4]; uint32_t version, nc, nk, ...
        uint32_t v;
        memcpy(&v, h + 12, 4);
        *nk = (int)std::min<uint32_t>(v, 1u << 20);
    }
    return IRMV_OK;
}

static void pose_prior_defaults(irmv_pose_prior *p);   // (pose ambiguity, below)

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
    if (cfg->point_source < 0 || cfg->point_source > IRMV_POINTS_REFINED) return fail(IRMV_ERR_ARG, "bad point_source");
    // The refined source needs the keypoint head: where the blob's header can be read without the GPU (a path, host memory)
    // a model without one is refused here, before any HIP call; a blob in device memory right after it has been fetched.
    if (cfg->point_source == IRMV_POINTS_REFINED) {
        int nk = -1;
        if (int rc = peek_blob_nk(*cfg, &nk)) return rc;
        if (nk >= 0 && nk < 8) return refined_needs_head();
    }
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
    e->sw = read_switches();
    pose_prior_defaults(&e->pose_prior);
    yaw_opts_defaults(&e->yaw_opts);
    pose_cov_opts_defaults(&e->posecov_opts);
    patch_opts_defaults(&e->patch_opts);
    track_opts_defaults(&e->track_opts);
    {
        TrackSlot ts{};   // stamp 0, camera pose identity
        ts.R[0] = ts.R[4] = ts.R[8] = 1.0;
        e->track_slots.assign((size_t)cfg->num_slots, ts);
    }
    e->up.assign((size_t)cfg->num_slots * 3, 0.0);
    for (int s = 0; s < cfg->num_slots; s++) e->up[3 * s + 1] = -1.0;   // a level camera: image y points down
    int rc = load_blob(e.get());
    e->cfg.weights_path = nullptr;  // caller-owned, not retained
    e->cfg.weights_blob = nullptr;
    if (rc) return rc;
    if (cfg->point_source == IRMV_POINTS_REFINED && e->nk < 8) return refined_needs_head();   // (nothing is allocated yet)
    TRY(build_engine(e.get()));
    TRY(autotune_convs(e.get()));
    finalize_head_fusion(e.get());
    TRY(build_head_groups(e.get()));
    build_step_plans(e.get(), e->views[IRMV_VIEW_WINDOW]);
    TRY(choose_sync_launch(e.get()));
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
int irmv::window_map(int full_w, int full_h, int win_w, int win_h, int rotate180, const double K[9], int x0, int y0, irmv_window_map_t *m)
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

// The tile grid of a tiled search, one axis: F the frame's extent, w the window's, ov the least overlap of neighbours.  The
// fewest tiles that cover F with that overlap, spread evenly: corner i is i (F - w) / (n - 1) rounded to nearest.
static int tile_axis(int F, int w, int ov, int *c, int cap)
{
    const int n = w == F ? 1 : (F - ov + (w - ov) - 1) / (w - ov);
    if (n > cap) return n;
    for (int i = 0; i < n; i++) c[i] = n == 1 ? 0 : (int)((2ll * i * (F - w) + (n - 1)) / (2ll * (n - 1)));
    return n;
}

extern "C" int irmv_tile_grid(const irmv_engine_cfg *cfg_in, int min_overlap_x, int min_overlap_y, int32_t *xy, int cap, int *n, int *nx, int *ny)
{
    if (!cfg_in || !n) return fail(IRMV_ERR_ARG, "cfg/n is null");
    irmv_engine_cfg full;
    if (int rc = resolve_cfg(cfg_in, &full)) return rc;
    if (full.win_width == 0) return fail(IRMV_ERR_ARG, "irmv_tile_grid: the configuration has no window (win_width, win_height)");
    if (min_overlap_x < 0 || min_overlap_x >= full.win_width || min_overlap_y < 0 || min_overlap_y >= full.win_height)
        return fail(IRMV_ERR_ARG, "irmv_tile_grid: the overlap must be in [0, window extent)");
    int cx[IRMV_MAX_TILES], cy[IRMV_MAX_TILES];
    const int gx = tile_axis(full.src_width, full.win_width, min_overlap_x, cx, IRMV_MAX_TILES);
    const int gy = tile_axis(full.src_height, full.win_height, min_overlap_y, cy, IRMV_MAX_TILES);
    if (gx > IRMV_MAX_TILES || gy > IRMV_MAX_TILES || gx * gy > IRMV_MAX_TILES)
        return fail(IRMV_ERR_ARG, "irmv_tile_grid: the grid has more than IRMV_MAX_TILES tiles");
    *n = gx * gy;
    if (nx) *nx = gx;
    if (ny) *ny = gy;
    if (!xy) return IRMV_OK;
    if (cap < gx * gy) return fail(IRMV_ERR_ARG, "irmv_tile_grid: cap is smaller than the grid");
    for (int iy = 0; iy < gy; iy++)
        for (int ix = 0; ix < gx; ix++) { xy[2 * (iy * gx + ix)] = cx[ix]; xy[2 * (iy * gx + ix) + 1] = cy[iy]; }
    return IRMV_OK;
}

// The slot's entries of the two device tables from e->win_org[slot] and its view: the corner always, the camera with the
// principal point moved by it in the window view and as configured in the frame view.  The caller has made sure no step of
// the slot is in flight.
int irmv::write_window(irmv_engine *e, int slot)
{
    irmv_window_map_t m;
    TRY(window_map(e->full_w, e->full_h, e->cfg.src_width, e->cfg.src_height, e->cfg.rotate180, e->cfg.camera_matrix, e->win_org[slot].x, e->win_org[slot].y, &m));
    const int2 b{m.bx0, m.by0};
    PnpConst pc = e->pnp_base;
    if (e->slot_view[slot] == IRMV_VIEW_WINDOW) { pc.cx = m.cx; pc.cy = m.cy; }
    HIP_TRY(hipMemcpy(e->win_dev + slot, &b, sizeof b, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->pnp_dev + slot, &pc, sizeof pc, hipMemcpyHostToDevice));
    return IRMV_OK;
}

// What the window and view entry points (`who`) ask of their arguments first: an engine, with a window, and a slot of it.
int irmv::check_window_slot(const irmv_engine *e, int slot, const char *who)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->window) return fail(IRMV_ERR_ARG, std::string(who) + ": the engine has no window (win_width, win_height)");
    if (slot < 0 || slot >= e->cfg.num_slots) return fail(IRMV_ERR_ARG, "slot out of range");
    return IRMV_OK;
}

extern "C" int irmv_engine_set_window(irmv_engine *e, int slot, int x0, int y0)
{
    TRY(check_window_slot(e, slot, "irmv_engine_set_window"));
    irmv_window_map_t m;
    TRY(window_map(e->full_w, e->full_h, e->cfg.src_width, e->cfg.src_height, e->cfg.rotate180, e->cfg.camera_matrix, x0, y0, &m));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read both tables
    e->win_org[slot] = int2{x0, y0};
    return write_window(e, slot);
}

extern "C" int irmv_engine_get_window(const irmv_engine *e, int slot, int *x0, int *y0, int *w, int *h)
{
    TRY(check_window_slot(e, slot, "irmv_engine_get_window"));
    if (x0) *x0 = e->win_org[slot].x;
    if (y0) *y0 = e->win_org[slot].y;
    if (w) *w = e->cfg.src_width;
    if (h) *h = e->cfg.src_height;
    return IRMV_OK;
}

// ---- search view --------------------------------------------------------------------
extern "C" int irmv_engine_set_view(irmv_engine *e, int slot, int view)
{
    TRY(check_window_slot(e, slot, "irmv_engine_set_view"));
    if (view != IRMV_VIEW_WINDOW && view != IRMV_VIEW_FRAME) return fail(IRMV_ERR_ARG, "unknown view (IRMV_VIEW_*)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (view == IRMV_VIEW_FRAME && !e->views[IRMV_VIEW_FRAME].built) {
        irmv_engine_cfg full = e->cfg;
        full.src_width = e->full_w; full.src_height = e->full_h;
        TRY(check_letterbox(full));
        TRY(irmv_engine_wait(e));   // every stream of the engine: the build appends to what steps read
        TRY(build_frame_view(e));
    }
    TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read its camera record
    if (e->slot_view[slot] == view) return IRMV_OK;
    e->slot_view[slot] = view;
    return write_window(e, slot);
}

extern "C" int irmv_engine_get_view(const irmv_engine *e, int slot, int *view, int *src_w, int *src_h)
{
    TRY(check_window_slot(e, slot, "irmv_engine_get_view"));
    const View &v = view_of(e, slot);
    if (view) *view = e->slot_view[slot];
    if (src_w) *src_w = v.src_w;
    if (src_h) *src_h = v.src_h;
    return IRMV_OK;
}

extern "C" int irmv_engine_debug_graph_count(const irmv_engine *e) { return e ? (int)e->graphs.size() : 0; }

// ---- extract parameters and Bayer ISP ------------------------------------------------
// T[c][v] = lut[c][min(255, (v gain[c] + 128) >> 8)] from the engine's current gains and LUT -> isp_table_dev.  The caller has
// made sure that nothing of this engine is in flight.
int irmv::write_isp_table(irmv_engine *e)
{
    uint8_t t[kBayerTableBytes];
    for (int c = 0; c < 3; c++)
        for (uint32_t v = 0; v < 256; v++) t[c * 256 + v] = e->isp_lut[c * 256 + std::min(255u, (v * e->isp_gain[c] + 128u) >> 8)];
    HIP_TRY(hipMemcpy(e->isp_table_dev, t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_point_source(const irmv_engine *e)
{
    if (!e) return -1;
    return e->refined ? IRMV_POINTS_REFINED : e->classical ? IRMV_POINTS_CLASSICAL : IRMV_POINTS_KEYPOINT_HEAD;
}

// ---- refined point source: the two live parameters ------------------------------------
// snap in (0, 4], roi_margin in [0, 64] source pixels; NaN fails both comparisons.  Host only.
static int check_refine(float snap, float roi_margin)
{
    if (!(snap > 0.f && snap <= 4.f)) return fail(IRMV_ERR_ARG, "irmv_engine_set_refine: snap must be in (0, 4]");
    if (!(roi_margin >= 0.f && roi_margin <= 64.f)) return fail(IRMV_ERR_ARG, "irmv_engine_set_refine: roi_margin must be in [0, 64]");
    return IRMV_OK;
}

extern "C" int irmv_engine_set_refine(irmv_engine *e, float snap, float roi_margin)
{
    TRY(check_refine(snap, roi_margin));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no launch in flight reads the pair
    e->refine = RefineParams{snap, roi_margin};
    if (e->refine_dev) HIP_TRY(hipMemcpy(e->refine_dev, &e->refine, sizeof e->refine, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_get_refine(const irmv_engine *e, float *snap, float *roi_margin)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (snap) *snap = e->refine.snap;
    if (roi_margin) *roi_margin = e->refine.roi_margin;
    return IRMV_OK;
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
    // captured steps of the classical and the refined mode carry these values as kernel arguments: re-capture on next use
    if (e->classical || e->refined) drop_graphs(e, false);
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
        drop_graphs(e, true);
        for (size_t i = 0; i < e->ops.size(); i++) {
            if (e->ops[i].kind != OP_DEMOSAIC) continue;
            snprintf(e->ops[i].kname, sizeof e->ops[i].kname, "%s", demosaic_kname(e));
            for (View &v : e->views)
                for (auto &plan : v.plans)
                    for (Launch &l : plan)
                        if (l.op == (int)i) l.name = e->ops[i].kname;
        }
    }
    return IRMV_OK;
}

// ---- class policy ----------------------------------------------------------------------
extern "C" int irmv_class_policy_uniform(float score_thr, int armor_size, irmv_class_policy *out)
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    if (!(score_thr > 0.f)) return fail(IRMV_ERR_ARG, "score_thr must be above 0 (>= 1: off)");
    if (armor_size != IRMV_ARMOR_SMALL && armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    for (int c = 0; c < 16; c++) { out->score_thr[c] = score_thr; out->plate[c] = (uint8_t)armor_size; }
    return IRMV_OK;
}

extern "C" int irmv_class_policy_enemy(int enemy_color, float score_thr, int armor_size, irmv_class_policy *out)
{
    if (enemy_color < -1 || enemy_color > 1) return fail(IRMV_ERR_ARG, "enemy_color must be 0 (blue), 1 (red) or -1 (both)");
    TRY(irmv_class_policy_uniform(score_thr, armor_size, out));
    // ArmorClass (armor.hpp): B1..BS = 0..6, R1..RS = 7..13.  The enemy's classes stay on, the own colour's are off.
    if (enemy_color >= 0)
        for (int c = 0; c < 7; c++) out->score_thr[(enemy_color == 0 ? 7 : 0) + c] = 1.0f;
    return IRMV_OK;
}

extern "C" int irmv_class_policy_table(const irmv_class_policy *p, int nc, float logit_thr[16], float *min_logit_thr)
{
    if (!p || !logit_thr || !min_logit_thr) return fail(IRMV_ERR_ARG, "null argument");
    if (p->struct_size != sizeof(irmv_class_policy)) return fail(IRMV_ERR_ARG, "irmv_class_policy.struct_size mismatch");
    if (nc < 1 || nc > 16) return fail(IRMV_ERR_ARG, "nc must be 1..16");
    for (int c = 0; c < nc; c++) {
        if (!(p->score_thr[c] > 0.f)) return fail(IRMV_ERR_ARG, "score_thr[" + std::to_string(c) + "] must be above 0 (>= 1: the class is off)");
        if (p->plate[c] != IRMV_ARMOR_SMALL && p->plate[c] != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "plate[" + std::to_string(c) + "] must be IRMV_ARMOR_SMALL or IRMV_ARMOR_LARGE");
    }
    float mn = INFINITY;
    for (int c = 0; c < 16; c++) {
        const float t = c < nc ? p->score_thr[c] : 1.0f;
        // (the arithmetic cfg.score_thr has always had: double on the float32 t, rounded once)
        logit_thr[c] = t >= 1.f ? INFINITY : (float)std::log((double)t / (1.0 - (double)t));
        mn = std::min(mn, logit_thr[c]);
    }
    *min_logit_thr = mn;
    return IRMV_OK;
}

// e->policy -> cls_dev[0] and its mute twin.  The caller has made sure that nothing of this engine is in flight.
int irmv::write_class_table(irmv_engine *e)
{
    ClassTable t[2] = {};
    TRY(irmv_class_policy_table(&e->policy, e->nc, t[0].thr, &t[0].min_thr));
    t[1].min_thr = INFINITY;
    for (int c = 0; c < kMaxClasses; c++) {
        t[0].plate[c] = t[1].plate[c] = c < e->nc ? e->policy.plate[c] : e->cfg.armor_size;
        t[1].thr[c] = INFINITY;
    }
    HIP_TRY(hipMemcpy(e->cls_dev, t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_set_class_policy(irmv_engine *e, const irmv_class_policy *p)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    irmv_class_policy np;
    if (p) {
        float thr[16], mn;
        TRY(irmv_class_policy_table(p, e->nc, thr, &mn));   // every check, before anything changes
        np = *p;
    } else {
        TRY(irmv_class_policy_uniform(e->cfg.score_thr, e->cfg.armor_size, &np));
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the table
    e->policy = np;
    return write_class_table(e);
}

extern "C" int irmv_engine_get_class_policy(const irmv_engine *e, irmv_class_policy *out)
{
    if (!e || !out) return fail(IRMV_ERR_ARG, "engine / out is null");
    *out = e->policy;
    return IRMV_OK;
}

// ---- pose ambiguity ---------------------------------------------------------------------
static void pose_prior_defaults(irmv_pose_prior *p)
{
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->mode = IRMV_POSE_MIN_ERR;
    p->ambiguity_ratio = 8.0;
    for (int c = 0; c < 16; c++) p->normal_up[c] = -0.25881904510252074;   // -sin 15 deg: a robot's plate
    p->normal_up_default = -0.25881904510252074;
}

// Host only; NaN fails every comparison
static int check_pose_prior(const irmv_pose_prior *p)
{
    if (p->struct_size != sizeof(irmv_pose_prior)) return fail(IRMV_ERR_ARG, "irmv_pose_prior.struct_size mismatch");
    if (p->mode != IRMV_POSE_MIN_ERR && p->mode != IRMV_POSE_PRIOR) return fail(IRMV_ERR_ARG, "irmv_pose_prior.mode: unknown mode (IRMV_POSE_*)");
    if (!(p->ambiguity_ratio >= 1.0)) return fail(IRMV_ERR_ARG, "irmv_pose_prior.ambiguity_ratio must be >= 1 (+inf allowed)");
    for (int c = 0; c < 16; c++)
        if (!(std::fabs(p->normal_up[c]) <= 1.0)) return fail(IRMV_ERR_ARG, "irmv_pose_prior.normal_up[" + std::to_string(c) + "] must be in [-1, 1]");
    if (!(std::fabs(p->normal_up_default) <= 1.0)) return fail(IRMV_ERR_ARG, "irmv_pose_prior.normal_up_default must be in [-1, 1]");
    return IRMV_OK;
}

// e->pose_prior -> prior_dev.  The caller has made sure that nothing of this engine is in flight.
static int write_pose_prior(irmv_engine *e)
{
    PosePrior t{};
    t.mode = e->pose_prior.mode;
    t.ratio = e->pose_prior.ambiguity_ratio;
    for (int c = 0; c < kMaxClasses; c++) t.s[c] = e->pose_prior.normal_up[c];
    t.s_default = e->pose_prior.normal_up_default;
    HIP_TRY(hipMemcpy(e->prior_dev, &t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

// The first irmv_engine_set_pose_prior: the alt records (device and pinned, zeroed), the two tables, and the one re-capture --
// the captured steps hold the kAlt = false kernel nodes.  Nothing of the engine is in flight.
static int enable_pose_alt(irmv_engine *e)
{
    const size_t n = (size_t)e->cfg.num_slots * e->cfg.max_det;
    // DevAlt: doubles, and two int32 flags (state, alt_ok) that only the host reads; nms_pnp_kernel<true> / light_extract write
    // the records of [0, num_dets), no kernel reads one
    TRY(dev_alloc(e, (void **)&e->alts.dev, n * sizeof(DevAlt), "alts_dev", mem_scratch(MEM_F64)));
    TRY(e->alts.pin(e, e->cfg.num_slots, e->cfg.max_det, "pinned alts_host"));
    TRY(dev_alloc(e, (void **)&e->prior_dev, sizeof(PosePrior), "prior_dev", mem_const(MEM_F64)));   // host-written tables, read when the kernel runs
    TRY(dev_alloc(e, (void **)&e->up_dev, e->up.size() * sizeof(double), "up_dev", mem_const(MEM_F64)));
    HIP_TRY(hipMemcpy(e->up_dev, e->up.data(), e->up.size() * sizeof(double), hipMemcpyHostToDevice));
    e->pose_alt = true;
    drop_graphs(e, false);
    return IRMV_OK;
}

extern "C" int irmv_engine_set_pose_prior(irmv_engine *e, const irmv_pose_prior *p)
{
    irmv_pose_prior np;
    if (p) {
        TRY(check_pose_prior(p));   // (the values first: a refused one never reaches the engine)
        np = *p;
    } else {
        pose_prior_defaults(&np);
    }
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the table, no graph is running
    if (!e->pose_alt) TRY(enable_pose_alt(e));
    e->pose_prior = np;
    TRY(write_pose_prior(e));
    return write_yaw_tables(e);   // (the constrained pose reads the classes' tilts)
}

extern "C" int irmv_engine_get_pose_prior(const irmv_engine *e, irmv_pose_prior *out)
{
    if (!e || !out) return fail(IRMV_ERR_ARG, "engine / out is null");
    *out = e->pose_prior;
    return IRMV_OK;
}

extern "C" int irmv_engine_set_up(irmv_engine *e, int slot, const double up[3])
{
    if (!up) return fail(IRMV_ERR_ARG, "up is null");
    const double len = std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
    if (!(len > 0.0 && len < INFINITY)) return fail(IRMV_ERR_ARG, "irmv_engine_set_up: the vector must be finite and non-zero");
    TRY(check_range(e, slot, 1));
    const double u[3] = {up[0] / len, up[1] / len, up[2] / len};
    if (e->pose_alt) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read the table
        HIP_TRY(hipMemcpy(e->up_dev + 3 * slot, u, sizeof u, hipMemcpyHostToDevice));
    }
    std::copy(u, u + 3, e->up.begin() + 3 * slot);
    if (e->yaw_op >= 0) {   // the constrained pose's basis of the slot
        if (!e->pose_alt) { HIP_TRY(hipSetDevice(e->cfg.device)); TRY(irmv_engine_wait_slots(e, slot, 1)); }
        TRY(write_yaw_tables(e, slot));
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_get_up(const irmv_engine *e, int slot, double up[3])
{
    TRY(check_range(e, slot, 1));
    if (!up) return fail(IRMV_ERR_ARG, "up is null");
    std::copy(e->up.begin() + 3 * slot, e->up.begin() + 3 * slot + 3, up);
    return IRMV_OK;
}

extern "C" int irmv_engine_pose_alts(irmv_engine *e, int slot, irmv_pose_alt *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (!e->pose_alt) return fail(IRMV_ERR_ARG, "irmv_engine_pose_alts: irmv_engine_set_pose_prior has not been called on this engine");
    static_assert(sizeof(DevAlt) == sizeof(irmv_pose_alt), "DevAlt is irmv_pose_alt");
    return e->alts.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_engine_get_bayer_isp(const irmv_engine *e, uint16_t gain_q8[3], uint8_t *lut)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->raw_dev) return fail(IRMV_ERR_ARG, "irmv_engine_get_bayer_isp: not a Bayer engine (src_format is IRMV_SRC_HWC8)");
    if (gain_q8) for (int i = 0; i < 3; i++) gain_q8[i] = e->isp_gain[i];
    if (lut) memcpy(lut, e->isp_lut, kBayerTableBytes);
    return IRMV_OK;
}

// ---- PnPSolver -------------------------------------------------------------------------
static void pnp_free(irmv_pnp *p)
{
    if (p->pts) (void)hipFree(p->pts);
    if (p->rvec) (void)hipFree(p->rvec);
    if (p->tvec) (void)hipFree(p->tvec);
    if (p->err) (void)hipFree(p->err);
    if (p->ok) (void)hipFree(p->ok);
    if (p->yaw) (void)hipFree(p->yaw);
    if (p->cov_poses) (void)hipFree(p->cov_poses);
    if (p->cov) (void)hipFree(p->cov);
    p->cov_poses = nullptr; p->cov = nullptr;
    p->yaw = nullptr;
    p->pts = nullptr; p->rvec = p->tvec = p->err = nullptr; p->ok = nullptr; p->cap = 0;
}

int pnp_reserve(irmv_pnp *p, int n)   // (engine_yaw.cpp's and engine_posecov.cpp's stand-alone calls reserve here too)
{
    if (n <= p->cap) return IRMV_OK;
    pnp_free(p);
    const int cap = std::max(n, 64);
    HIP_TRY(hipMalloc((void **)&p->pts, (size_t)cap * 32));
    HIP_TRY(hipMalloc((void **)&p->rvec, (size_t)cap * 48));
    HIP_TRY(hipMalloc((void **)&p->tvec, (size_t)cap * 48));
    HIP_TRY(hipMalloc((void **)&p->err, (size_t)cap * 16));
    HIP_TRY(hipMalloc((void **)&p->ok, (size_t)cap * 4));
    HIP_TRY(hipMalloc((void **)&p->yaw, (size_t)cap * sizeof(DevYaw)));
    HIP_TRY(hipMalloc((void **)&p->cov_poses, (size_t)cap * 6 * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&p->cov, (size_t)cap * sizeof(DevPoseCov)));
    p->cap = cap;
    return IRMV_OK;
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
    TRY(pnp_reserve(p, n));
    HIP_TRY(hipMemcpyAsync(p->pts, img_pts, (size_t)n * 32, hipMemcpyHostToDevice, p->stream));
    launch_pnp_only(p->c, p->pts, n, armor_size, p->rvec, p->tvec, p->ok, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rvec, p->rvec, (size_t)n * 24, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(tvec, p->tvec, (size_t)n * 24, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(ok, p->ok, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return IRMV_OK;
}

extern "C" int irmv_pnp_solve2(irmv_pnp *p, const float *img_pts, int n, int armor_size, double *rvec, double *tvec, double *err, int32_t *ok)
{
    if (!p || !img_pts || !rvec || !tvec || !err || !ok || n < 0) return fail(IRMV_ERR_ARG, "null argument");
    if (armor_size != IRMV_ARMOR_SMALL && armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(p->device));
    TRY(pnp_reserve(p, n));
    HIP_TRY(hipMemcpyAsync(p->pts, img_pts, (size_t)n * 32, hipMemcpyHostToDevice, p->stream));
    launch_pnp_both(p->c, p->pts, n, armor_size, p->rvec, p->tvec, p->err, p->ok, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rvec, p->rvec, (size_t)n * 48, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(tvec, p->tvec, (size_t)n * 48, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(err, p->err, (size_t)n * 16, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(ok, p->ok, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return IRMV_OK;
}
