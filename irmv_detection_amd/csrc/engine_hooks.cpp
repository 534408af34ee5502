// Everything that looks into an engine from outside a step: read-backs, the debug_* calls, the LDS fill / probe, the conv and
// op test hooks, the light trace and the profiler.
#include "engine_internal.hpp"

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

extern "C" int irmv_engine_debug_write_cand_bits(irmv_engine *e, int slot, const uint32_t *words, int n)
{
    TRY(check_range(e, slot, 1));
    if (!e->sparse_head) return fail(IRMV_ERR_ARG, "write_cand_bits: this engine has no sparse head");
    if (!words || n != e->cand_words) return fail(IRMV_ERR_ARG, "write_cand_bits: the word count is not the engine's");
    for (int wd = 0; wd < n; wd++) {   // (cand_list_kernel guards `an < A` itself: that guard is not for a test to lean on)
        const int lo = wd * 32;
        const uint32_t past = lo >= e->A ? 0xffffffffu : (e->A - lo >= 32 ? 0u : 0xffffffffu << (e->A - lo));
        if (words[wd] & past) return fail(IRMV_ERR_ARG, "write_cand_bits: a bit at or past the last anchor is set");
    }
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpy(e->cand_bits + (size_t)slot * e->cand_words, words, (size_t)n * sizeof(unsigned int), hipMemcpyHostToDevice));
    return IRMV_OK;
}

// the level's OP_BOXG op; -1: none
static int boxg_of_level(const irmv_engine *e, int level)
{
    for (size_t i = 0; i < e->ops.size(); i++)
        if (e->ops[i].kind == OP_BOXG && e->ops[i].level == level) return (int)i;
    return -1;
}

extern "C" int irmv_engine_debug_write_cand_lists(irmv_engine *e, int level, int first, int count, const int32_t *counts, const int32_t *entries)
{
    TRY(check_range(e, first, count));
    if (level < 0 || level > 2 || !e->boxg_list || boxg_of_level(e, level) < 0) return fail(IRMV_ERR_ARG, "write_cand_lists: the level has no box gather op");
    if (!counts || !entries) return fail(IRMV_ERR_ARG, "write_cand_lists: counts / entries is null");
    const int hw = e->lvl_hw[level];
    for (int i = 0; i < count; i++)   // (box_gather_kernel clamps both itself: those clamps are not for a test to lean on)
        if (counts[i] < 0 || counts[i] > hw) return fail(IRMV_ERR_ARG, "write_cand_lists: a count outside [0, H * W]");
    for (size_t i = 0; i < (size_t)count * hw; i++)
        if (entries[i] < 0 || entries[i] >= hw) return fail(IRMV_ERR_ARG, "write_cand_lists: an entry outside [0, H * W)");
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t S = (size_t)e->cfg.num_slots;   // (cand_list_args' addresses)
    HIP_TRY(hipMemcpy(e->boxg_list + (size_t)e->lvl_base[level] * S + (size_t)first * hw, entries, (size_t)count * hw * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->boxg_count + (size_t)level * S + first, counts, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_rotated_image(irmv_engine *e, int slot, uint8_t *dst)
{
    TRY(check_range(e, slot, 1));
    if (!dst) return fail(IRMV_ERR_ARG, "dst is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const View &v = view_of(e, slot);
    // the slot's step in flight may run on another compute stream and still read the device frame load_frame rewrites (its
    // pinned slot may be the producer's again since irmv_engine_wait_upload); other slots stay in flight
    TRY(irmv_engine_wait_slots(e, slot, 1));
    TRY(load_frame(e, slot, e->stream));
    launch_rotate180(v.frames + (size_t)slot * v.frame_bytes, v.rot_dev, v.src_w, v.src_h, e->stream);
    HIP_TRY(hipMemcpyAsync(dst, v.rot_dev, v.frame_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// ---- debug images (include/irmv_hip.h, "debug images"; k_render.hip) -----------------------------------------------------
// THE glyph table: irmv_render_glyph reads it, and the device font is built from it.
static const struct { char ch; uint8_t rows[7]; } kRenderGlyphs[] = {
    {'B', {0x1e, 0x11, 0x11, 0x1e, 0x11, 0x11, 0x1e}}, {'R', {0x1e, 0x11, 0x11, 0x1e, 0x14, 0x12, 0x11}},
    {'O', {0x0e, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e}}, {'S', {0x0f, 0x10, 0x10, 0x0e, 0x01, 0x01, 0x1e}},
    {'U', {0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e}}, {'N', {0x11, 0x19, 0x15, 0x13, 0x11, 0x11, 0x11}},
    {'K', {0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11}}, {'W', {0x11, 0x11, 0x11, 0x15, 0x15, 0x1b, 0x11}},
    {'1', {0x04, 0x0c, 0x04, 0x04, 0x04, 0x04, 0x0e}}, {'2', {0x0e, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1f}},
    {'3', {0x1e, 0x01, 0x01, 0x0e, 0x01, 0x01, 0x1e}}, {'4', {0x02, 0x06, 0x0a, 0x12, 0x1f, 0x02, 0x02}},
    {'5', {0x1f, 0x10, 0x1e, 0x01, 0x01, 0x11, 0x0e}}};
constexpr int kRenderGlyphCount = (int)(sizeof kRenderGlyphs / sizeof *kRenderGlyphs);
static_assert(kRenderGlyphCount <= 16, "RenderFont::glyph");
// ArmorClass names (reference include/irmv_detection/armor.hpp:7), UNKNOWN last
static const char *const kRenderNames[IRMV_NUM_CLASSES + 1] = {"B1", "B2", "B3", "B4", "B5", "BO", "BS", "R1", "R2", "R3", "R4", "R5", "RO", "RS", "UNKNOWN"};

static int render_glyph_index(int ch)
{
    for (int i = 0; i < kRenderGlyphCount; i++)
        if (kRenderGlyphs[i].ch == ch) return i;
    return -1;
}

extern "C" int irmv_render_glyph(int ch, uint8_t rows[7])
{
    const int i = render_glyph_index(ch);
    if (i < 0 || !rows) return fail(IRMV_ERR_ARG, "render_glyph: no such glyph, or rows is null");
    memcpy(rows, kRenderGlyphs[i].rows, 7);
    return IRMV_OK;
}

static int check_render_scale(int scale)
{
    if (scale != 1 && scale != 2 && scale != 4) return fail(IRMV_ERR_ARG, "render: scale must be 1, 2 or 4");
    return IRMV_OK;
}

extern "C" int irmv_engine_render_dims(const irmv_engine *e, int slot, int scale, int *w, int *h)
{
    TRY(check_range(e, slot, 1));
    TRY(check_render_scale(scale));
    if (!w || !h) return fail(IRMV_ERR_ARG, "render_dims: w / h is null");
    const View &v = view_of(e, slot);
    *w = v.src_w / scale;
    *h = v.src_h / scale;
    return IRMV_OK;
}

// The scratch of irmv_engine_render, made by its first call: mark records, the font, the picture.
static int ensure_render(irmv_engine *e)
{
    if (e->render_out) return IRMV_OK;
    RenderFont f;
    memset(&f, 0, sizeof f);
    for (int i = 0; i < kRenderGlyphCount; i++) memcpy(f.glyph[i], kRenderGlyphs[i].rows, 7);
    for (int c = 0; c <= IRMV_NUM_CLASSES; c++) {
        f.len[c] = (uint8_t)strlen(kRenderNames[c]);
        for (int k = 0; k < f.len[c]; k++) f.name[c][k] = (uint8_t)render_glyph_index(kRenderNames[c][k]);
    }
    if (!e->render_marks) TRY(dev_alloc(e, (void **)&e->render_marks, (size_t)e->cfg.max_det * sizeof(RenderMark), "render_marks", mem_const(MEM_INDEX)));   // the host uploads the n marks a call draws (cls indexes the font)
    if (!e->render_font) TRY(dev_alloc(e, (void **)&e->render_font, sizeof(RenderFont), "render_font", mem_const(MEM_INDEX)));
    HIP_TRY(hipMemcpy(e->render_font, &f, sizeof f, hipMemcpyHostToDevice));
    e->render_marks_host.resize((size_t)e->cfg.max_det);
    TRY(dev_alloc(e, (void **)&e->render_out, std::max(e->frame_bytes, e->full_bytes), "render_out", mem_scratch(MEM_U8)));   // the picture: written by the kernel, copied to the host
    return IRMV_OK;
}

// A mark coordinate: v truncated toward zero, the corner subtracted, floor-divided by the scale; false where v has none
static bool render_coord(float v, int org, int scale, int32_t *out)
{
    if (!std::isfinite(v) || std::fabs(v) >= 16777216.f) return false;
    const int t = (int)v - org;
    *out = t >= 0 ? t / scale : -((-t + scale - 1) / scale);
    return true;
}

extern "C" int irmv_engine_render(irmv_engine *e, int slot, const irmv_render_opts *o, const irmv_det *dets, int n, uint8_t *dst)
{
    TRY(check_range(e, slot, 1));
    if (!o || !dst) return fail(IRMV_ERR_ARG, "render: opts / dst is null");
    if (o->struct_size != sizeof(irmv_render_opts)) return fail(IRMV_ERR_ARG, "render: opts.struct_size is not sizeof(irmv_render_opts)");
    if (o->kind != IRMV_RENDER_COLOR && o->kind != IRMV_RENDER_BINARY) return fail(IRMV_ERR_ARG, "render: unknown kind");
    TRY(check_render_scale(o->scale));
    if (o->marks & ~(IRMV_MARK_BOXES | IRMV_MARK_LABELS | IRMV_MARK_ARMORS)) return fail(IRMV_ERR_ARG, "render: unknown mark bits");
    if (o->reserved[0] || o->reserved[1] || o->reserved[2]) return fail(IRMV_ERR_ARG, "render: reserved fields must be 0");
    if (o->binary_threshold < -1 || o->binary_threshold > 255) return fail(IRMV_ERR_ARG, "render: binary_threshold must be -1..255");
    const bool last = !dets && n == -1;
    if (!last && (n < 0 || n > e->cfg.max_det || (n > 0 && !dets))) return fail(IRMV_ERR_ARG, "render: n must be 0..max_det with dets set, or -1 with dets null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    TRY(ensure_render(e));
    std::vector<irmv_det> own;
    if (last) {
        own.resize((size_t)e->cfg.max_det);
        TRY(irmv_engine_results(e, slot, own.data(), e->cfg.max_det, &n));
        dets = own.data();
    }
    hipStream_t st = e->stream;
    const View &v = view_of(e, slot);
    const int s = o->scale, ox = v.crop ? e->win_org[slot].x : 0, oy = v.crop ? e->win_org[slot].y : 0;
    for (int i = 0; i < n; i++) {
        const irmv_det &d = dets[i];
        RenderMark &m = e->render_marks_host[(size_t)i];
        memset(&m, 0, sizeof m);
        m.cls = d.class_id >= 0 && d.class_id < IRMV_NUM_CLASSES ? d.class_id : IRMV_NUM_CLASSES;
        if (render_coord(d.xyxy[0], ox, s, &m.x1) && render_coord(d.xyxy[1], oy, s, &m.y1) && render_coord(d.xyxy[2], ox, s, &m.x2) && render_coord(d.xyxy[3], oy, s, &m.y2))
            m.flags |= (o->marks & IRMV_MARK_BOXES ? kRenderBox : 0) | (o->marks & IRMV_MARK_LABELS ? kRenderLabel : 0);
        bool pts = d.armor_valid == 1 && (o->marks & IRMV_MARK_ARMORS);
        for (int k = 0; k < 4 && pts; k++) pts = render_coord(d.kpts[2 * k], ox, s, &m.px[k]) && render_coord(d.kpts[2 * k + 1], oy, s, &m.py[k]);
        if (pts) m.flags |= kRenderArmor;
    }
    TRY(load_frame(e, slot, st));
    if (n > 0) HIP_TRY(hipMemcpyAsync(e->render_marks, e->render_marks_host.data(), (size_t)n * sizeof(RenderMark), hipMemcpyHostToDevice, st));
    RenderArgs a{};
    a.frame = v.frames + (size_t)slot * v.frame_bytes;
    a.dst = e->render_out;
    a.marks = e->render_marks;
    a.font = e->render_font;
    a.W = v.src_w; a.H = v.src_h; a.ow = v.src_w / s; a.oh = v.src_h / s;
    a.rotate180 = e->cfg.rotate180 ? 1 : 0;
    a.scale = s;
    a.binary = o->kind == IRMV_RENDER_BINARY;
    a.threshold = o->binary_threshold >= 0 ? o->binary_threshold : e->cfg.binary_threshold;
    a.n = n;
    if (a.ow > 0 && a.oh > 0) {
        launch_render_view(a, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst, e->render_out, (size_t)a.ow * a.oh * 3, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return IRMV_OK;
}

static_assert(sizeof(irmv_light_rec) == sizeof(LightTraceRec) && sizeof(irmv_light_trace) == sizeof(LightTrace) &&
                  offsetof(irmv_light_trace, starts) == offsetof(LightTrace, starts) && offsetof(irmv_light_trace, points) == offsetof(LightTrace, points) &&
                  offsetof(irmv_light_trace, recs) == offsetof(LightTrace, recs) && offsetof(irmv_light_rec, length) == offsetof(LightTraceRec, length) &&
                  IRMV_LIGHT_MAX_CONTOURS == kLightMaxContours && IRMV_LIGHT_POINTS_CAP == kLightPointsCap,
              "irmv_light_trace is LightTrace");

// The guided launch's device state on an engine that is not a refined one, made by its first irmv_engine_refine_points: the
// parameter pair and one slot's worth of prior.
static int ensure_refine(irmv_engine *e)
{
    if (!e->refine_dev) {
        RefineParams *p = nullptr;
        TRY(dev_alloc(e, (void **)&p, sizeof(RefineParams), "refine_params", mem_const(MEM_F32)));
        HIP_TRY(hipMemcpy(p, &e->refine, sizeof e->refine, hipMemcpyHostToDevice));
        e->refine_dev = p;
    }
    if (!e->refine_kpts) TRY(dev_alloc(e, (void **)&e->refine_kpts, (size_t)e->cfg.max_det * 8 * sizeof(float), "refine_kpts", mem_scratch(MEM_F32)));   // (as build_post_stage's)
    return IRMV_OK;
}

// irmv_engine_extract_armors; trace != nullptr: irmv_engine_light_trace (the kernel also records its stages);
// kpts != nullptr: irmv_engine_refine_points (the guided instantiation on explicit boxes and keypoints)
static int extract_armors(irmv_engine *e, int slot, const float *xyxy, const float *kpts, int n, irmv_light_trace *trace, irmv_det *out)
{
    TRY(check_range(e, slot, 1));
    if (n < 0 || n > e->cfg.max_det || (n > 0 && (!xyxy || !out))) return fail(IRMV_ERR_ARG, "n must be 0..max_det with xyxy/out set");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    hipStream_t st = e->stream;
    if (kpts) TRY(ensure_refine(e));
    // the trace of a hook call: zeroed in front of every launch, written by the kernel, read by the host, which indexes by its
    // counts and starts -- so nothing but zero is valid in every word
    if (trace && !e->light_trace_dev) TRY(dev_alloc(e, (void **)&e->light_trace_dev, (size_t)e->cfg.max_det * sizeof(LightTrace), "light_trace", mem_scratch_index(0u)));
    if (trace) HIP_TRY(hipMemsetAsync(e->light_trace_dev, 0, (size_t)n * sizeof(LightTrace), st));
    TRY(load_frame(e, slot, st));
    // a window engine takes the boxes in full result coordinates: in the window view window-local for the kernel, the corner
    // back onto its points
    const View &v = view_of(e, slot);
    const bool shift = v.crop;
    const float ox = shift ? (float)e->win_org[slot].x : 0.f, oy = shift ? (float)e->win_org[slot].y : 0.f;
    std::vector<float> local;
    if (shift) {
        local.assign(xyxy, xyxy + (size_t)n * 4);
        for (size_t j = 0; j < local.size(); j++) local[j] -= (j & 1) ? oy : ox;
        HIP_TRY(hipMemcpyAsync(e->light_boxes, local.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));   // (`local` is pageable memory of this call)
        if (kpts) {
            local.assign(kpts, kpts + (size_t)n * 8);
            for (size_t j = 0; j < local.size(); j++) local[j] -= (j & 1) ? oy : ox;
            HIP_TRY(hipMemcpyAsync(e->refine_kpts, local.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    } else {
        HIP_TRY(hipMemcpyAsync(e->light_boxes, xyxy, (size_t)n * 16, hipMemcpyHostToDevice, st));
        if (kpts) HIP_TRY(hipMemcpyAsync(e->refine_kpts, kpts, (size_t)n * 32, hipMemcpyHostToDevice, st));
    }
    LightArgs a = light_args(e, v, slot);
    // the classical instantiation on a refined engine too; the guided one on any engine (slot 0's share of the prior buffer:
    // nothing is in flight, and a step gathers its prior anew)
    a.refine = kpts ? e->refine_dev : nullptr;
    a.kpts = kpts ? e->refine_kpts : nullptr;
    a.dets = e->light_dets_dev;
    a.labels = v.light_labels;
    a.points = e->light_points;
    a.hulls = e->light_hulls;
    a.num_dets = nullptr;
    a.n_boxes = n;
    a.boxes = e->light_boxes;
    a.alts = nullptr;   // explicit boxes have no class: normal_up_default, and no alt record
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
        det_pose(d, shift, ox, oy, o);
        if (kpts) o.reserved = d.pad_;   // the refine flag
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_extract_armors(irmv_engine *e, int slot, const float *xyxy, int n, irmv_det *out)
{
    return extract_armors(e, slot, xyxy, nullptr, n, nullptr, out);
}

extern "C" int irmv_engine_refine_points(irmv_engine *e, int slot, const float *xyxy, const float *kpts, int n, irmv_light_trace *trace, irmv_det *out)
{
    if (n > 0 && !kpts) return fail(IRMV_ERR_ARG, "kpts is null");
    return extract_armors(e, slot, xyxy, kpts, n, trace, out);
}

extern "C" int irmv_engine_light_trace(irmv_engine *e, int slot, const float *xyxy, int n, irmv_light_trace *trace, irmv_det *out)
{
    if (n > 0 && !trace) return fail(IRMV_ERR_ARG, "trace is null");
    return extract_armors(e, slot, xyxy, nullptr, n, trace, out);
}

extern "C" int irmv_light_limits(int32_t out[4])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    out[0] = kLightMaxContours; out[1] = kLightPointsCap; out[2] = kLightLdsImage; out[3] = kLightLdsPoints;
    return IRMV_OK;
}

extern "C" int irmv_post_limits(int32_t out[16])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    post_limits(out);
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

// Run one of the two LDS kernels over `wgs` workgroups on a quiet device: a zeroed device buffer of `bytes` for it to write, copied to `out`.
template <class F> static int debug_lds_run(size_t bytes, void *out, F &&launch)
{
    void *d = nullptr;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMalloc(&d, bytes));
    hipError_t e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = launch(static_cast<uint32_t *>(d));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(e);
    return IRMV_OK;
}

extern "C" int irmv_debug_lds_fill(uint32_t pattern32)
{
    int wgs = 0;
    if (int rc = debug_lds_geometry(&wgs)) return rc;
    uint32_t bad = 0;
    TRY(debug_lds_run(sizeof bad, &bad, [&](uint32_t *d) { return launch_lds_fill(pattern32, d, wgs, nullptr); }));
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
    return debug_lds_run((size_t)wgs * 4 * sizeof(uint32_t), out, [&](uint32_t *d) { return launch_lds_probe(pattern32, word, d, wgs, nullptr); });
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
    TRY(enqueue_step(e, Step{STEP_MATERIALIZE, slot, 1}, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->head_stale[slot] = 0;   // (the finals and the keypoint layers have written every head row)
    e->branch_stale[slot] = 0; // (... and the box branches' gated first convs their whole tensors)
    return IRMV_OK;
}

// The head of a slot whose last step stored candidate rows only (sparse_head): the read-back step runs the branches' finals
// and the keypoint layers as layers, which write every row -- the same bits the carriers compute.  A head written through
// irmv_engine_write_head since that step is not stale and stays as written.
int irmv::ensure_dense_head(irmv_engine *e, int slot)
{
    return e->head_stale[slot] ? materialize_fused(e, slot) : IRMV_OK;
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

extern "C" int irmv_engine_write_tensor(irmv_engine *e, const char *name, int first, int count, const void *src, size_t bytes)
{
    TRY(check_range(e, first, count));
    if (!name) return fail(IRMV_ERR_ARG, "name is null");
    auto it = e->tensor_idx.find(name);
    if (it == e->tensor_idx.end()) return fail(IRMV_ERR_ARG, std::string("no tensor named ") + name);
    const Tensor &t = e->tensors[it->second];
    const size_t need = t.slot_elems * t.esize() * count;
    if (!src || bytes != need) return fail(IRMV_ERR_ARG, "write_tensor: buffer size does not match the slot range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    // the dense state first (what ensure_dense_head and read_tensor's branch_stale path run), whatever tensor is written: the
    // read-back step would otherwise run later, over the written values
    for (int s = first; s < first + count; s++) {
        if (e->head_stale[s] || e->branch_stale[s]) TRY(materialize_fused(e, s));
        e->head_stale[s] = 0;
        e->branch_stale[s] = 0;
    }
    HIP_TRY(hipMemcpy(t.slot(first), src, need, hipMemcpyHostToDevice));
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

template <size_t N> static void put_name(char (&dst)[N], const std::string &s) { snprintf(dst, N, "%s", s.c_str()); }

// A segment as the listing calls report it.  whole: a segment without a channel count of its own stands for the rest of its
// tensor (irmv_engine_ops); otherwise it is no segment (irmv_engine_conv_ops).
static void put_seg(const irmv_engine *e, irmv_conv_seg &d, const SegRef &s, bool whole)
{
    memset(&d, 0, sizeof d);
    if (s.t < 0 || (s.C == 0 && !whole)) return;
    put_name(d.tensor, e->tensors[s.t].name);
    d.coff = s.coff; d.C = s.C > 0 ? s.C : e->tensors[s.t].C - s.coff; d.shift = s.shift;
}

// IRMV_RUN_POISON / _POISON_ONLY of a hook's run: all-ones bytes (a NaN in fp16 and in fp32) over channels [coff, coff + C) of
// tensor t on slots [first, first + count), what the run must write.
constexpr uint32_t kRunPoisons = IRMV_RUN_POISON | IRMV_RUN_POISON_ONLY;
static int poison_output(irmv_engine *e, const Tensor &t, int coff, int C, int first, int count)
{
    if (coff + C > t.C) return fail(IRMV_ERR_ARG, "output channels out of range");
    HIP_TRY(hipMemset2DAsync(static_cast<char *>(t.slot(first)) + (size_t)coff * t.esize(), (size_t)t.C * t.esize(), 0xff, (size_t)C * t.esize(), (size_t)count * t.H * t.W, e->stream));
    return IRMV_OK;
}

extern "C" int irmv_engine_conv_ops(irmv_engine *e, irmv_conv_op *ops, int cap, int *n)
{
    if (!e || !n) return fail(IRMV_ERR_ARG, "engine / n is null");
    int k = 0;
    for (size_t i = 0; i < e->ops.size(); i++) {
        const Op &op = e->ops[i];
        if (op.kind != OP_CONV) continue;
        if (ops && k < cap) {
            irmv_conv_op &r = ops[k];
            memset(&r, 0, sizeof r);
            r.op = (int32_t)i;
            put_name(r.layer, op.layer);
            r.ks = op.cfg.ks; r.stride = op.cfg.stride; r.act = op.cfg.act; r.out_f32 = op.cfg.out_f32;
            r.cin = op.cin; r.cout = op.cout; r.cout_pad = op.cout_pad;
            r.Hin = op.Hin; r.Win = op.Win; r.Hout = op.Hout; r.Wout = op.Wout;
            put_seg(e, r.s0, op.s0, false);
            put_seg(e, r.s1, op.s1, false);
            if (op.res_t >= 0) put_seg(e, r.res, SegRef{op.res_t, op.res_coff, op.cout, 0}, false);
            const Tensor &ot = e->tensors[op.out_t];
            put_name(r.out_tensor, ot.name);
            r.out_coff = op.out_coff;
            r.out_lazy = e->lazy_tensors.count(ot.name) ? 1 : 0;
            r.fused = op.fuse_next >= 0;
            r.tune_fused = op.tune_fuse[0] >= 0 || op.tune_fuse[1] >= 0;
            const int f = op.fuse_next >= 0 ? op.fuse_next : std::max(op.tune_fuse[0], op.tune_fuse[1]);
            if (f >= 0) {
                const Op &o2 = e->ops[f];
                put_name(r.fuse_layer, o2.layer);
                put_name(r.fuse_tensor, e->tensors[o2.out_t].name);
                r.fuse_coff = o2.out_coff; r.fuse_cout = o2.cout; r.fuse_cout_pad = o2.cout_pad;
            }
            put_name(r.kname, op.kname);
            put_name(r.kname_one, op.kname_one);
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
    cands = tune_candidates(o, v.a, tune_count, v.want_fuse, v.lds_ok, e->sw.tune, e->num_cus);
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
    if (flags & kRunPoisons) {
        // the real output channels: the fused 1x1's slice of the head when the run carries it (the 3x3's own output then never
        // leaves the registers)
        const Op &w = v.a.n2 > 0 ? e->ops[o.fuse_next] : real;
        TRY(poison_output(e, e->tensors[w.out_t], w.out_coff, w.cout, first, count));
    }
    if (flags & IRMV_RUN_POISON_ONLY) { HIP_TRY(hipStreamSynchronize(e->stream)); return IRMV_OK; }
    if (!run_conv(o, c, v.a, count, e->stream)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        return IRMV_DECLINED;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// ---- per-op test hooks (tests/test_gpu_graph_ops.py) ---------------------------------
static const char *op_kind_name(OpKind k)   // (in OpKind's order)
{
    static const char *const names[] = {"pre", "conv0", "conv", "pool", "nms", "light", "front", "c2f2", "c2f32", "dw", "shuffle", "scan", "bneck", "kpt3", "boxg", "demosaic", "crop", "meter", "yaw", "patch", "number", "pose_cov"};
    static_assert(sizeof names / sizeof *names == OP_POSECOV + 1, "a name per OpKind (OP_POSECOV is the last)");
    return (unsigned)k <= OP_POSECOV ? names[k] : "?";
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
    for (size_t i = 0; ops && i < e->ops.size() && (int)i < cap; i++) {
        const Op &op = e->ops[i];
        irmv_graph_op &r = ops[i];
        memset(&r, 0, sizeof r);
        r.op = (int32_t)i;
        put_name(r.kind, op_kind_name(op.kind));
        put_name(r.layer, op.layer);
        put_name(r.kname, op.kname);
        put_seg(e, r.s0, op.kind == OP_POOL ? SegRef{op.out_t, 0, e->tensors[op.out_t].C / 4, 0} : op.s0, true);
        put_seg(e, r.s1, op.s1, true);
        int t, coff, C;
        op_output(e, op, &t, &coff, &C);
        if (t >= 0) {
            put_name(r.out_tensor, e->tensors[t].name);
            r.out_coff = coff; r.out_C = C;
        }
        r.fused_away = op.fused_away ? 1 : 0;
    }
    *n = (int)e->ops.size();
    return IRMV_OK;
}

// The OP_KPT3 op whose branch a batched step's launch of OP_BOXG op `op` computes too (Launch::kpt, the same in every view);
// -1: the launch is box only, or no batched step gathers.
static int boxg_kpt(const irmv_engine *e, int op)
{
    for (const Launch &l : e->views[0].plans[STEP_BATCH])
        if (l.op == op && l.group < 0) return l.kpt;
    return -1;
}

// What a fused op's launch writes and reads, from the argument builders of engine_step.cpp (c2f2_args, c2f32_args, bneck_args,
// kpt3_args, boxg_args) and the kernels behind them; false: op is no fused op.
struct FusedIo { std::vector<int> sub; std::vector<SegRef> writes, reads; };
static bool fused_io(const irmv_engine *e, const Op &op, FusedIo &io)
{
    io = FusedIo{};
    for (int k = 0; k < 4; k++) if (op.sub[k] >= 0) io.sub.push_back(op.sub[k]);
    auto seg = [&](const SegRef &s) { if (s.t >= 0 && s.C > 0) io.reads.push_back(s); };
    switch (op.kind) {
    case OP_C2F2:    // the block input -> the block output; cat and tmp stay on chip
        seg(op.s0);
        io.writes.push_back(SegRef{op.out_t, 0, e->ops[op.sub[3]].cout, 0});
        return true;
    case OP_C2F32:   // mode 0: input -> output; 1: input -> y0 | y1 | y2 of the concat buffer; 2: y0 | y1 | y2 -> output
        if (op.mode != 2) { seg(e->ops[op.sub[0]].s0); seg(e->ops[op.sub[0]].s1); }
        else seg(SegRef{op.res_t, 0, 96, 0});
        if (op.mode == 1) io.writes.push_back(SegRef{op.res_t, 0, 96, 0});
        else io.writes.push_back(SegRef{op.out_t, 0, e->ops[op.sub[3]].cout, 0});
        return true;
    case OP_BNECK: { // A: slice y_in of the concat buffer -> the next slice; B: the slices up to and including y_in -> the block output
        const Op &m1 = e->ops[op.sub[0]], &m2 = e->ops[op.sub[1]];
        if (op.sub[2] < 0) {
            seg(m1.s0);
            io.writes.push_back(SegRef{m2.out_t, m2.out_coff, m2.cout, 0});
        } else {
            const Op &c2 = e->ops[op.sub[2]];
            seg(SegRef{op.res_t, 0, m1.s0.coff + m1.s0.C, 0});
            io.writes.push_back(SegRef{c2.out_t, c2.out_coff, c2.cout, 0});
        }
        return true;
    }
    case OP_KPT3: {  // the level's input -> the keypoint channels of its head records
        const Op &o2 = e->ops[op.sub[2]];
        seg(e->ops[op.sub[0]].s0);
        io.writes.push_back(SegRef{o2.out_t, o2.out_coff, o2.cout_pad, 0});   // (the final's padding rows too: 16 floats of a record)
        return true;
    }
    case OP_BOXG: {  // the level's input -> the box channels of its head records at the candidate anchors, and the keypoint channels where the branch rides
        const Op &o2 = e->ops[op.sub[2]];
        seg(e->ops[op.sub[0]].s0);
        io.writes.push_back(SegRef{o2.out_t, o2.out_coff, o2.cout, 0});
        const int k = boxg_kpt(e, (int)(&op - e->ops.data()));
        if (k >= 0) {
            const Op &k2 = e->ops[e->ops[k].sub[2]];
            io.writes.push_back(SegRef{k2.out_t, k2.out_coff, k2.cout_pad, 0});   // (kpt3's: the final's padding rows too)
        }
        return true;
    }
    default: return false;
    }
}

extern "C" int irmv_engine_op_io(irmv_engine *e, int op, irmv_op_io *out)
{
    if (!e || !out) return fail(IRMV_ERR_ARG, "engine / io is null");
    if (op < 0 || op >= (int)e->ops.size()) return fail(IRMV_ERR_ARG, "no such op");
    FusedIo io;
    if (!fused_io(e, e->ops[op], io)) return fail(IRMV_ERR_ARG, std::string("op_io describes c2f2, c2f32, bneck, kpt3 and boxg ops, not ") + op_kind_name(e->ops[op].kind));
    memset(out, 0, sizeof *out);
    out->op = op;
    out->n_sub = (int32_t)io.sub.size(); out->n_writes = (int32_t)io.writes.size(); out->n_reads = (int32_t)io.reads.size();
    for (size_t i = 0; i < io.sub.size(); i++) out->sub[i] = io.sub[i];
    for (size_t i = 0; i < io.writes.size(); i++) put_seg(e, out->writes[i], io.writes[i], false);
    for (size_t i = 0; i < io.reads.size(); i++) put_seg(e, out->reads[i], io.reads[i], false);
    return IRMV_OK;
}

extern "C" int irmv_engine_run_op(irmv_engine *e, int op, int first, int count, uint32_t flags)
{
    TRY(check_range(e, first, count));
    if (op < 0 || op >= (int)e->ops.size()) return fail(IRMV_ERR_ARG, "no such op");
    const Op &o = e->ops[op];
    FusedIo io;
    const bool fused = fused_io(e, o, io);
    if (!fused && o.kind != OP_CONV0 && o.kind != OP_POOL && o.kind != OP_DW && o.kind != OP_SHUF)
        return fail(IRMV_ERR_ARG, std::string("run_op runs conv0, pool, dw, shuffle, c2f2, c2f32, bneck, kpt3 and boxg ops, not ") + op_kind_name(o.kind));
    const bool boxg = o.kind == OP_BOXG;
    if (!boxg && (flags & ~kRunPoisons)) return fail(IRMV_ERR_ARG, "run_op: flags other than the poison flags are a boxg op's");
    if (boxg && (flags & ~(kRunPoisons | IRMV_RUN_BOX_ONLY | IRMV_RUN_WRITTEN_LISTS | 0xffff0000u))) return fail(IRMV_ERR_ARG, "run_op: unknown flag bits");
    if (boxg && (!e->sparse_head || !e->boxg_list)) return fail(IRMV_ERR_ARG, "run_op: a boxg op needs the sparse head's bitmap and the candidate lists");
    if (boxg && ((flags & IRMV_RUN_BOX_ONLY) || boxg_kpt(e, op) < 0) && io.writes.size() > 1) io.writes.resize(1);   // (box only: the keypoint channels are not this run's)
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    if (fused) TRY(slots_view(e, first, count, nullptr));
    if ((flags & kRunPoisons) && fused) {
        for (const SegRef &w : io.writes) TRY(poison_output(e, e->tensors[w.t], w.coff, w.C, first, count));
    } else if (flags & kRunPoisons) {
        int t, coff, C;
        op_output(e, o, &t, &coff, &C);
        TRY(poison_output(e, e->tensors[t], coff, C, first, count));
    }
    if (flags & IRMV_RUN_POISON_ONLY) { HIP_TRY(hipStreamSynchronize(e->stream)); return IRMV_OK; }
    Launch l;   // (a plain launch of the op: no group, no fusion, no gate)
    l.op = op;
    if (boxg) {   // cand_list_kernel in front unless the lists are the caller's; the keypoint branch where a batched step links it
        l.sparse = true;
        l.cand_list = !(flags & IRMV_RUN_WRITTEN_LISTS);
        l.kpt = (flags & IRMV_RUN_BOX_ONLY) ? -1 : boxg_kpt(e, op);
        l.grid = (int)(flags >> 16);
    }
    const Step step{count == 1 ? STEP_ONE : STEP_BATCH, first, count};
    TRY(launch_op(e, view_of(e, first), l, step, post_args(e, view_of(e, first), step), 0u, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// ---- device-memory residue hooks (tests/test_gpu_mem_residue.py) ------------------------
extern "C" int irmv_engine_debug_allocs(irmv_engine *e, irmv_mem_range *recs, int cap, int *n)
{
    if (!e || !n) return fail(IRMV_ERR_ARG, "engine / n is null");
    *n = (int)e->dev_allocs.size();
    if (!recs) return IRMV_OK;
    if (cap < *n) return fail(IRMV_ERR_ARG, "debug_allocs: buffer too small");
    for (size_t i = 0; i < e->dev_allocs.size(); i++) {
        const DevRange &r = e->dev_allocs[i];
        irmv_mem_range &o = recs[i];
        memset(&o, 0, sizeof o);
        put_name(o.name, r.name);
        o.mem_class = r.tag.cls; o.kind = r.tag.kind; o.index_max = r.tag.index_max;
        o.bytes = r.bytes; o.base = (uint64_t)(uintptr_t)r.base;
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_debug_read_cand_counts(irmv_engine *e, int32_t *counts, int cap, int *n)
{
    if (!e || !n) return fail(IRMV_ERR_ARG, "engine / n is null");
    *n = e->cand_counts ? e->cfg.num_slots : 0;
    if (!counts || *n == 0) return IRMV_OK;
    if (cap < *n) return fail(IRMV_ERR_ARG, "read_cand_counts: buffer too small");
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpy(counts, e->cand_counts, (size_t)*n * sizeof(int), hipMemcpyDeviceToHost));
    return IRMV_OK;
}

extern "C" int irmv_engine_debug_read_mem(irmv_engine *e, int range, uint64_t offset, void *dst, uint64_t bytes)
{
    if (!e || !dst) return fail(IRMV_ERR_ARG, "engine / dst is null");
    if (range < 0 || range >= (int)e->dev_allocs.size()) return fail(IRMV_ERR_ARG, "debug_read_mem: no such range");
    const DevRange &r = e->dev_allocs[(size_t)range];
    if (offset > r.bytes || bytes > r.bytes - offset) return fail(IRMV_ERR_ARG, "debug_read_mem: outside range " + r.name);
    TRY(irmv_engine_wait(e));
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpy(dst, static_cast<const char *>(r.base) + offset, bytes, hipMemcpyDeviceToHost));
    return IRMV_OK;
}

// `bytes` at p (2-byte aligned) <- the 32-bit word v, whose halfwords are equal: words, then a halfword, then a byte
static int fill_range(void *p, size_t bytes, uint32_t v, hipStream_t st)
{
    char *c = static_cast<char *>(p);
    if (((uintptr_t)c & 2) && bytes >= 2) { HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)c, (unsigned short)v, 1, st)); c += 2; bytes -= 2; }
    if (bytes / 4) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c, (int)v, bytes / 4, st));
    c += bytes / 4 * 4;
    if (bytes & 2) { HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)c, (unsigned short)v, 1, st)); c += 2; }
    if (bytes & 1) HIP_TRY(hipMemsetD8Async((hipDeviceptr_t)c, (unsigned char)v, 1, st));
    return IRMV_OK;
}

// The channels of every tensor that some op declares as written: op_output of every op and the writes of the fused ones --
// what irmv_engine_ops and irmv_engine_op_io report.
static std::vector<std::vector<char>> written_channels(const irmv_engine *e)
{
    std::vector<std::vector<char>> w(e->tensors.size());
    for (size_t t = 0; t < w.size(); t++) w[t].assign((size_t)e->tensors[t].C, 0);
    auto mark = [&](int t, int coff, int C) { for (int c = std::max(coff, 0); t >= 0 && c < coff + C && c < e->tensors[t].C; c++) w[t][c] = 1; };
    for (const Op &op : e->ops) {
        int t, coff, C;
        op_output(e, op, &t, &coff, &C);
        mark(t, coff, C);
        FusedIo io;
        if (fused_io(e, op, io)) for (const SegRef &s : io.writes) mark(s.t, s.coff, s.C);
    }
    return w;
}

extern "C" int irmv_engine_debug_fill_mem(irmv_engine *e, uint32_t pattern32, uint64_t *filled)
{
    if (!e || !filled) return fail(IRMV_ERR_ARG, "engine / filled is null");
    if ((pattern32 >> 16) != (pattern32 & 0xffffu)) return fail(IRMV_ERR_ARG, "debug_fill_mem: the two halfwords of the pattern must be equal");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    hipStream_t st = e->stream;
    const int S = e->cfg.num_slots;
    uint64_t total = 0;
    for (const DevRange &r : e->dev_allocs) {
        if (r.tag.cls != MEM_SCRATCH) continue;
        if (r.tag.kind == MEM_INDEX) {   // whole words of the largest value valid in every indexing use
            if (r.bytes & 3) return fail(IRMV_ERR_ARG, "debug_fill_mem: INDEX range " + r.name + " is no whole number of words");
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)r.base, (int)(pattern32 == 0 ? 0u : r.tag.index_max), r.bytes / 4, st));
        } else TRY(fill_range(r.base, r.bytes, pattern32, st));
        total += r.bytes;
    }
    // The written channels of every tensor.  A tensor written whole is one fill.  Any other is read back, patterned on the
    // written channels in a buffer of this call and written again, so its pad channels keep exactly what they held.  (The
    // path of IRMV_RUN_POISON, hipMemset2DAsync, takes a byte value, and these patterns are halfwords.)
    const auto w = written_channels(e);
    std::vector<uint16_t> host;
    for (size_t ti = 0; ti < w.size(); ti++) {
        const Tensor &t = e->tensors[ti];
        const size_t n_written = (size_t)std::count(w[ti].begin(), w[ti].end(), (char)1), rows = (size_t)S * t.H * t.W;
        const size_t hw = t.esize() / 2;   // halfwords per element
        if (n_written == 0) continue;
        if (n_written == (size_t)t.C) TRY(fill_range(t.base, rows * t.C * t.esize(), pattern32, st));
        else {
            host.resize(rows * t.C * hw);
            HIP_TRY(hipMemcpy(host.data(), t.base, host.size() * 2, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < rows; r++)
                for (int c = 0; c < t.C; c++)
                    if (w[ti][c]) for (size_t k = 0; k < hw; k++) host[(r * t.C + c) * hw + k] = (uint16_t)pattern32;
            HIP_TRY(hipMemcpy(t.base, host.data(), host.size() * 2, hipMemcpyHostToDevice));
        }
        total += n_written * t.esize() * rows;
    }
    HIP_TRY(hipStreamSynchronize(st));
    *filled = total;
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
    const DevFrameOut &fo = *e->fout.host_at(slot);
    const DevDet *d = e->dets.host_at(slot);
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

// The events of a profiled step -- launch i of the plan runs between ev[2 i] and ev[2 i + 1] --, destroyed however
// irmv_engine_profile returns.
struct ProfileEvents {
    std::vector<hipEvent_t> ev;
    ~ProfileEvents() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};

extern "C" int irmv_engine_profile(irmv_engine *e, int first, int count, irmv_kernel_stat *stats, int cap, int *n)
{
    TRY(check_range(e, first, count));
    if (!n) return fail(IRMV_ERR_ARG, "n is null");
    int view;
    TRY(slots_view(e, first, count, &view));
    HIP_TRY(hipSetDevice(e->cfg.device));
    // Eager replay of the step's launches on the engine stream, every kernel bracketed by an event
    // pair.  The kernels are idempotent and are launched kProfileRepeat times inside their bracket: an event pair around ONE launch also times ~4 us of
    // command-processor hand-over, which would read as kernel time on these 5-80 us kernels.
    // (Event-record nodes inside a captured graph cannot be read back with hipEventElapsedTime on
    // ROCm 7.2: "invalid resource handle".)
    TRY(irmv_engine_wait(e));
    const StepKind kind = count == 1 ? STEP_ONE : STEP_BATCH;
    const std::vector<Launch> &plan = e->views[view].plans[kind];
    ProfileEvents pe;
    pe.ev.resize(2 * plan.size(), nullptr);
    for (hipEvent_t &x : pe.ev) HIP_TRY(hipEventCreate(&x));
    TRY(enqueue_step(e, Step{kind, first, count}, e->stream, kProfileRepeat, &pe.ev));   // (a window engine crops out of its device frames, as a submit without IRMV_SUBMIT_H2D does)
    mark_stepped(e, first, count);
    TRY(copy_out(e, first, count));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < plan.size(); i++) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pe.ev[2 * i], pe.ev[2 * i + 1]));
        const Launch &l = plan[i];
        if ((int)i < cap && stats) {
            irmv_kernel_stat &st = stats[i];
            memset(&st, 0, sizeof st);
            put_name(st.name, l.name);
            put_name(st.layer, l.layer);
            st.flops = l.flops * count;
            st.bytes = l.bytes * count + l.launch_bytes;
            st.ms = l.once ? ms : ms / (float)kProfileRepeat;
        }
    }
    *n = (int)plan.size();
    return IRMV_OK;
}
