// Frame metering (include/irmv_hip.h, "frame metering"; k_meter.hip): the argument checks and the map, the host helpers that
// read a record, the on-demand call, and the switch that puts the op into the engine's steps.
#include "engine_internal.hpp"

static_assert(sizeof(MeterStats) == sizeof(irmv_frame_stats) && sizeof(irmv_frame_stats) % 16 == 0 && offsetof(MeterStats, n) == offsetof(irmv_frame_stats, n) &&
                  offsetof(MeterStats, rect) == offsetof(irmv_frame_stats, rect) && offsetof(MeterStats, domain) == offsetof(irmv_frame_stats, domain) &&
                  offsetof(MeterStats, step) == offsetof(irmv_frame_stats, step),
              "MeterStats is irmv_frame_stats");
static_assert(kMeterView == IRMV_METER_VIEW && kMeterRaw == IRMV_METER_RAW, "the kernels' domains are the header's");

// Every check of the options; bayer: the engine (or configuration) has a raw frame.  No GPU call.
static int check_meter_opts(const irmv_meter_opts *o, bool bayer)
{
    if (!o) return fail(IRMV_ERR_ARG, "metering: opts is null");
    if (o->struct_size != sizeof(irmv_meter_opts)) return fail(IRMV_ERR_ARG, "metering: opts.struct_size is not sizeof(irmv_meter_opts)");
    if (o->domain != IRMV_METER_VIEW && o->domain != IRMV_METER_RAW) return fail(IRMV_ERR_ARG, "metering: unknown domain (IRMV_METER_*)");
    if (o->domain == IRMV_METER_RAW && !bayer) return fail(IRMV_ERR_ARG, "metering: IRMV_METER_RAW needs a Bayer engine (src_format is IRMV_SRC_HWC8)");
    if (o->step != 1 && o->step != 2 && o->step != 4) return fail(IRMV_ERR_ARG, "metering: step must be 1, 2 or 4");
    if (o->w < 0 || o->h < 0) return fail(IRMV_ERR_ARG, "metering: w and h must not be negative");
    if ((o->w == 0) != (o->h == 0)) return fail(IRMV_ERR_ARG, "metering: w and h must both be 0 (the whole view) or both be at least 1");
    if (o->reserved[0] || o->reserved[1]) return fail(IRMV_ERR_ARG, "metering: reserved fields must be 0");
    return IRMV_OK;
}

static MeterParams meter_params(const irmv_meter_opts &o) { return MeterParams{1, o.domain, o.x0, o.y0, o.w, o.h, o.step, 0}; }

extern "C" int irmv_meter_map(const irmv_engine_cfg *cfg_in, const irmv_meter_opts *o, int view, int win_x0, int win_y0, irmv_meter_map_t *out)
{
    if (!cfg_in || !out) return fail(IRMV_ERR_ARG, "cfg/out is null");
    irmv_engine_cfg c;
    TRY(resolve_cfg(cfg_in, &c));
    TRY(check_meter_opts(o, c.src_format != IRMV_SRC_HWC8));
    if (view != IRMV_VIEW_WINDOW && view != IRMV_VIEW_FRAME) return fail(IRMV_ERR_ARG, "unknown view (IRMV_VIEW_*)");
    const bool window = c.win_width > 0;
    if (view == IRMV_VIEW_FRAME && !window) return fail(IRMV_ERR_ARG, "irmv_meter_map: IRMV_VIEW_FRAME needs a configuration with a window");
    int vw = c.src_width, vh = c.src_height, cx = 0, cy = 0;
    if (window) {
        irmv_window_map_t m;
        TRY(window_map(c.src_width, c.src_height, c.win_width, c.win_height, c.rotate180, c.camera_matrix, win_x0, win_y0, &m));
        if (view == IRMV_VIEW_WINDOW) { vw = c.win_width; vh = c.win_height; cx = m.bx0; cy = m.by0; }
    }
    const MeterGeom g = meter_geometry(meter_params(*o), vw, vh, c.rotate180 ? 1 : 0, cx, cy);
    memset(out, 0, sizeof *out);
    for (int i = 0; i < 4; i++) out->rect[i] = g.rect[i];
    out->region[0] = g.bx; out->region[1] = g.by; out->region[2] = g.bw; out->region[3] = g.bh;
    out->phase[0] = g.px; out->phase[1] = g.py;
    out->grid[0] = g.nx; out->grid[1] = g.ny;
    const uint32_t s = (uint32_t)g.nx * (uint32_t)g.ny;
    const bool raw = o->domain == IRMV_METER_RAW;   // a cell: one R, two G, one B site
    out->n[0] = s; out->n[1] = raw ? 2 * s : s; out->n[2] = s; out->n[3] = raw ? 4 * s : s;
    return IRMV_OK;
}

extern "C" int irmv_meter_limits(int32_t out[8])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    const int32_t v[8] = {kMeterRowsPerBlock, kMeterBlocksMax, kMeterLdsBytes, kMeterThreads, kMeterBatchFrames, kMeterBlocksBatch, 0, 0};
    for (int i = 0; i < 8; i++) out[i] = v[i];
    return IRMV_OK;
}

// ---- what a record says (host only) -------------------------------------------------------------------------------------
typedef unsigned __int128 u128;

static int check_stats_row(const irmv_frame_stats *s, int row)
{
    if (!s) return fail(IRMV_ERR_ARG, "stats is null");
    if (row < 0 || row > 3) return fail(IRMV_ERR_ARG, "stats: row must be 0..3");
    return IRMV_OK;
}

static int check_stats_range(int lo, int hi)
{
    if (lo < 0 || lo > 255 || hi < 0 || hi > 255) return fail(IRMV_ERR_ARG, "stats: lo and hi must be 0..255");
    return IRMV_OK;
}

// S = sum v h[v], N = sum h[v] over lo <= v <= hi: both fit 64 bits (h[v] < 2^32)
static void range_sums(const irmv_frame_stats *s, int row, int lo, int hi, uint64_t *S, uint64_t *N)
{
    *S = *N = 0;
    for (int v = lo; v <= hi; v++) { *S += (uint64_t)v * s->hist[row][v]; *N += s->hist[row][v]; }
}

extern "C" int irmv_stats_mean_q8(const irmv_frame_stats *s, int row, int lo, int hi, uint64_t *mean_q8, uint64_t *count)
{
    TRY(check_stats_row(s, row));
    TRY(check_stats_range(lo, hi));
    if (!mean_q8 || !count) return fail(IRMV_ERR_ARG, "stats: mean_q8 / count is null");
    uint64_t S, N;
    range_sums(s, row, lo, hi, &S, &N);
    *count = N;
    *mean_q8 = N ? (uint64_t)(((u128)256 * S + N / 2) / N) : 0;
    return IRMV_OK;
}

static int stats_percentile(const irmv_frame_stats *s, int row, uint64_t num, uint64_t den, int *value)
{
    TRY(check_stats_row(s, row));
    if (!value) return fail(IRMV_ERR_ARG, "stats: value is null");
    if (den == 0 || num > den) return fail(IRMV_ERR_ARG, "stats: the percentile needs den > 0 and num <= den");
    if (s->n[row] == 0) return fail(IRMV_ERR_ARG, "stats: the row has no sample");
    const u128 want = (u128)num * s->n[row];
    uint64_t cum = 0;
    for (int v = 0; v < 256; v++) {
        cum += s->hist[row][v];
        if ((u128)cum * den >= want) { *value = v; return IRMV_OK; }
    }
    *value = 255;   // (a record whose n is not the sum of its histogram)
    return IRMV_OK;
}

extern "C" int irmv_stats_percentile(const irmv_frame_stats *s, int row, uint64_t num, uint64_t den, int *value) { return stats_percentile(s, row, num, den, value); }

extern "C" int irmv_stats_gray_world(const irmv_frame_stats *s, int lo, int hi, uint16_t gain_q8[3])
{
    if (!s || !gain_q8) return fail(IRMV_ERR_ARG, "stats / gain_q8 is null");
    TRY(check_stats_range(lo, hi));
    if (s->domain != IRMV_METER_RAW) return fail(IRMV_ERR_ARG, "irmv_stats_gray_world: the record is not an IRMV_METER_RAW one");
    uint64_t S[3], N[3];
    for (int c = 0; c < 3; c++) range_sums(s, c, lo, hi, &S[c], &N[c]);
    uint16_t g[3] = {0, 256, 0};
    for (int c = 0; c < 3; c += 2) {
        const u128 d = (u128)S[c] * N[1];
        if (d == 0) return fail(IRMV_ERR_ARG, "irmv_stats_gray_world: no R, G or B mass inside [lo, hi]");
        const u128 q = ((u128)256 * S[1] * N[c] + d / 2) / d;
        g[c] = (uint16_t)(q < 1023 ? (uint64_t)q : 1023u);
    }
    memcpy(gain_q8, g, sizeof g);
    return IRMV_OK;
}

extern "C" int irmv_stats_exposure_q8(const irmv_frame_stats *s, int row, uint64_t num, uint64_t den, int target, int *ratio_q8)
{
    if (!ratio_q8) return fail(IRMV_ERR_ARG, "stats: ratio_q8 is null");
    if (target < 0 || target > 255) return fail(IRMV_ERR_ARG, "stats: target must be 0..255");
    int p = 0;
    TRY(stats_percentile(s, row, num, den, &p));
    const int r = (256 * target + p / 2) / std::max(p, 1);
    *ratio_q8 = std::min(std::max(r, 16), 4096);
    return IRMV_OK;
}

// ---- the engine ------------------------------------------------------------------------------------------------------------
// The scratch every metering call needs, made by the first: the partials slab (every launch rewrites what it reads), the two
// parameter records (off), the device records (zero).
static int ensure_meter(irmv_engine *e)
{
    if (e->meter.dev) return IRMV_OK;
    const size_t S = (size_t)e->cfg.num_slots;
    // partial histograms: 32-bit counts that the second kernel of a launch sums -- values, never indices
    if (!e->meter_slab) TRY(dev_alloc(e, (void **)&e->meter_slab, S * kMeterBlocksMax * 1024 * sizeof(uint32_t), "meter_slab", mem_scratch(MEM_F32)));
    // the options, written by the host alone (a rectangle: meter_geometry clips it to the view)
    if (!e->meter_params_dev) TRY(dev_alloc(e, (void **)&e->meter_params_dev, 2 * sizeof(MeterParams), "meter_params", mem_const(MEM_INDEX)));
    HIP_TRY(hipMemset(e->meter_params_dev, 0, 2 * sizeof(MeterParams)));
    MeterStats *st = nullptr;
    // the records: counts, the clipped rectangle and the echo of the options, written by the summing kernel, read by the host
    TRY(dev_alloc(e, (void **)&st, (S + 1) * sizeof(MeterStats), "meter_stats", mem_scratch(MEM_F32)));
    HIP_TRY(hipMemset(st, 0, (S + 1) * sizeof(MeterStats)));
    e->meter.dev = st;
    return IRMV_OK;
}

extern "C" int irmv_engine_meter(irmv_engine *e, int slot, const irmv_meter_opts *o, irmv_frame_stats *out)
{
    TRY(check_range(e, slot, 1));
    TRY(check_meter_opts(o, e->raw_dev != nullptr));
    if (!out) return fail(IRMV_ERR_ARG, "metering: out is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    TRY(ensure_meter(e));
    hipStream_t st = e->stream;
    const View &v = view_of(e, slot);
    const MeterParams p = meter_params(*o);
    HIP_TRY(hipMemcpy(e->meter_params_dev + 1, &p, sizeof p, hipMemcpyHostToDevice));
    TRY(load_frame(e, slot, st));
    MeterStats *rec = e->meter.dev + e->cfg.num_slots;   // (the record behind the steps')
    launch_frame_meter(meter_args(e, v, slot, e->meter_params_dev + 1, rec), 1, e->sw.meter_merge, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, rec, sizeof(MeterStats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return IRMV_OK;
}

// The first irmv_engine_set_metering with options: the pinned records, the op and the one re-capture -- the captured steps do
// not hold the meter's nodes.  Nothing of the engine is in flight.
static int enable_metering(irmv_engine *e)
{
    TRY(e->meter.pin(e, e->cfg.num_slots, 1, "pinned meter_stats_host"));   // (the steps' records: still zero, as ensure_meter left them)
    append_op(e, OP_METER);
    drop_graphs(e, true);   // (run_post's graphs have no meter node and stay)
    return IRMV_OK;
}

extern "C" int irmv_engine_set_metering(irmv_engine *e, const irmv_meter_opts *o)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (o) TRY(check_meter_opts(o, e->raw_dev != nullptr));   // (the values first: a refused one never reaches the engine)
    if (!o && e->meter_op < 0) return IRMV_OK;                // off, and never on: nothing to do
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the record, no graph is running
    TRY(ensure_meter(e));
    if (e->meter_op < 0) TRY(enable_metering(e));
    MeterParams p{};
    if (o) { p = meter_params(*o); e->meter_opts = *o; }
    e->meter_on = o != nullptr;
    HIP_TRY(hipMemcpy(e->meter_params_dev, &p, sizeof p, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_get_metering(const irmv_engine *e, irmv_meter_opts *o, int *on)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (on) *on = e->meter_on ? 1 : 0;
    if (o && e->meter_on) *o = e->meter_opts;
    return IRMV_OK;
}

extern "C" int irmv_engine_frame_stats(irmv_engine *e, int slot, irmv_frame_stats *out)
{
    TRY(check_range(e, slot, 1));
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    if (e->meter_op < 0) return fail(IRMV_ERR_ARG, "irmv_engine_frame_stats: irmv_engine_set_metering has not been called on this engine");
    memcpy(out, e->meter.host_at(slot), sizeof *out);
    return IRMV_OK;
}
