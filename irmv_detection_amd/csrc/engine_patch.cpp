// Plate patches (include/irmv_hip.h, "plate patches"; k_patch.hip): the option checks, the table the kernel reads and the
// call that rewrites it, the switch that puts the op into the engine's steps, the step's launch, the records' way to the
// caller, and the on-demand call on explicit points.  Compiled with -ffp-contract=off like the kernel's module; the host does
// no arithmetic of the model.
#include "engine_internal.hpp"

static_assert(sizeof(DevPatch) == sizeof(irmv_plate_patch) && sizeof(irmv_plate_patch) == 592 &&
                  offsetof(DevPatch, state) == offsetof(irmv_plate_patch, state) && offsetof(DevPatch, bar_sum) == offsetof(irmv_plate_patch, bar_sum) &&
                  offsetof(DevPatch, sum) == offsetof(irmv_plate_patch, sum) && sizeof(DevPatch) % 4 == 0,
              "DevPatch is irmv_plate_patch");
static_assert(kPatchW == IRMV_PATCH_W && kPatchH == IRMV_PATCH_H && kPatchW % 4 == 0, "header and kernel disagree");
static_assert(2 * (kPatchRowsMax + 1) <= 64, "the bars' points are one a lane");

void irmv::patch_opts_defaults(irmv_patch_opts *o)
{
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->enable = 0;
    o->span[0] = 32; o->span[1] = 54;
    o->light_rows = 12;
    o->top = 7;
}

static int check_patch_opts(const irmv_patch_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "patches: opts is null");
    if (o->struct_size != sizeof(irmv_patch_opts)) return fail(IRMV_ERR_ARG, "patches: opts.struct_size is not sizeof(irmv_patch_opts)");
    if (o->enable != 0 && o->enable != 1) return fail(IRMV_ERR_ARG, "patches: enable must be 0 or 1");
    for (int k = 0; k < 2; k++)
        if (o->span[k] < kPatchSpanMin || o->span[k] > kPatchSpanMax || (o->span[k] - kPatchW) % 2 != 0)
            return fail(IRMV_ERR_ARG, "patches: span must be 20 .. 128 with span - 20 even");
    if (o->light_rows < 1 || o->light_rows > kPatchRowsMax) return fail(IRMV_ERR_ARG, "patches: light_rows must be 1 .. 28");
    if (o->top < 0 || o->top > kPatchTopMax) return fail(IRMV_ERR_ARG, "patches: top must be 0 .. 27");
    if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(IRMV_ERR_ARG, "patches: reserved must be 0");
    return IRMV_OK;
}

// e->patch_opts -> the table (made by the first call that needs one).  The caller has made sure that no step in flight reads it.
int irmv::write_patch_table(irmv_engine *e)
{
    // host-written, read when the kernel runs
    if (!e->patch_table_dev) TRY(dev_alloc(e, (void **)&e->patch_table_dev, sizeof(PatchTable), "patch_table", mem_const(MEM_INDEX)));
    PatchTable t{};
    t.enable = e->patch_opts.enable; t.span[0] = e->patch_opts.span[0]; t.span[1] = e->patch_opts.span[1];
    t.light_rows = e->patch_opts.light_rows; t.top = e->patch_opts.top;
    HIP_TRY(hipMemcpy(e->patch_table_dev, &t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

// The first irmv_engine_set_patches: the records (device and pinned, zeroed), the op and the one re-capture -- no captured
// step holds the patch node.  Nothing of the engine is in flight.
int irmv::enable_patches(irmv_engine *e)
{
    const size_t n = (size_t)e->cfg.num_slots * e->cfg.max_det;
    // DevPatch: bytes and counts that only the host reads; patch_step_kernel writes every word of the records of [0, num_dets)
    // where it is enabled, no kernel reads one
    TRY(dev_alloc(e, (void **)&e->patch.dev, n * sizeof(DevPatch), "patch_dev", mem_scratch(MEM_U8)));
    TRY(e->patch.pin(e, e->cfg.num_slots, e->cfg.max_det, "pinned patch_host"));
    append_op(e, OP_PATCH);
    drop_graphs(e, false);   // (run_post's graphs too: the op stands behind their NMS)
    return IRMV_OK;
}

extern "C" int irmv_engine_set_patches(irmv_engine *e, const irmv_patch_opts *o)
{
    TRY(check_patch_opts(o));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the table, no graph is running
    if (e->patch_op < 0) TRY(enable_patches(e));
    if (!o->enable) TRY(e->patch.zero(e->cfg.num_slots));   // nothing writes the records from here on: none of an earlier step is left for a later enable to show
    e->patch_opts = *o;
    return write_patch_table(e);
}

extern "C" int irmv_engine_get_patches(const irmv_engine *e, irmv_patch_opts *o)
{
    if (!e || !o) return fail(IRMV_ERR_ARG, "engine / opts is null");
    *o = e->patch_opts;
    return IRMV_OK;
}

// A step's patches: they read the records of pa (where the step's NMS or light extraction wrote them) and the slots' frames
// exactly where light_args points the light extraction -- the view's device frames, which the step's upload (and crop, and
// demosaic) filled in front of its first layer on the same stream --, and go where the DevDet records go (Records::step_at).
void irmv::launch_patch(const irmv_engine *e, const View &v, const Step &s, const PostArgs &pa, hipStream_t st)
{
    PatchArgs a{};
    a.frames = v.frames + (size_t)s.first * v.frame_bytes;
    a.frame_bytes = v.frame_bytes;
    a.W = v.src_w; a.H = v.src_h; a.rotate180 = e->cfg.rotate180 ? 1 : 0;
    a.dets = pa.dets; a.max_det = e->cfg.max_det;
    a.num_dets = reinterpret_cast<const int *>(pa.fout);
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.table = e->patch_table_dev;
    a.out = e->patch.step_at(e, s);
    launch_patch_step(a, s.count, st);
}

extern "C" int irmv_engine_plate_patches(irmv_engine *e, int slot, irmv_plate_patch *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (e->patch_op < 0) return fail(IRMV_ERR_ARG, "irmv_engine_plate_patches: irmv_engine_set_patches has not been called on this engine");
    // (disabled: the kernel returns at once and set_patches has zeroed the records, so they stay all zero until the first step
    // after the next enable)
    return e->patch.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_engine_patches_at(irmv_engine *e, int slot, const float *kpts, const int32_t *armor_size, int n, irmv_plate_patch *out)
{
    if (n < 0 || n > kMaxDetCap || (n > 0 && (!kpts || !armor_size || !out))) return fail(IRMV_ERR_ARG, "patches_at: n must be 0..IRMV_MAX_DET_CAP with kpts/armor_size/out set");
    for (int i = 0; i < n; i++)
        if (armor_size[i] != IRMV_ARMOR_SMALL && armor_size[i] != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "patches_at: bad armor_size");
    TRY(check_range(e, slot, 1));
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    hipStream_t st = e->stream;
    if (!e->patch_table_dev) TRY(write_patch_table(e));
    // the call's buffers: the host uploads the n quads and sizes a call reads (a size indexes span[2]), the kernel writes
    // every word of the n records the host copies out
    if (!e->patch_at_kpts) TRY(dev_alloc(e, (void **)&e->patch_at_kpts, (size_t)kMaxDetCap * 8 * sizeof(float), "patch_at_kpts", mem_scratch(MEM_F32)));
    if (!e->patch_at_sizes) TRY(dev_alloc(e, (void **)&e->patch_at_sizes, (size_t)kMaxDetCap * sizeof(int32_t), "patch_at_sizes", mem_scratch_index(1u)));
    if (!e->patch_at_out) TRY(dev_alloc(e, (void **)&e->patch_at_out, (size_t)kMaxDetCap * sizeof(DevPatch), "patch_at_out", mem_scratch(MEM_U8)));
    TRY(load_frame(e, slot, st));
    // a window engine takes the points in full result coordinates: window-local for the kernel in the window view
    const View &v = view_of(e, slot);
    const float ox = v.crop ? (float)e->win_org[slot].x : 0.f, oy = v.crop ? (float)e->win_org[slot].y : 0.f;
    std::vector<float> local(kpts, kpts + (size_t)n * 8);
    if (v.crop)
        for (size_t j = 0; j < local.size(); j++) local[j] -= (j & 1) ? oy : ox;
    HIP_TRY(hipMemcpyAsync(e->patch_at_kpts, local.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->patch_at_sizes, armor_size, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (`local` is pageable memory of this call)
    PatchArgs a{};
    a.frames = v.frames + (size_t)slot * v.frame_bytes;
    a.frame_bytes = v.frame_bytes;
    a.W = v.src_w; a.H = v.src_h; a.rotate180 = e->cfg.rotate180 ? 1 : 0;
    a.max_det = e->cfg.max_det;
    a.table = e->patch_table_dev;
    a.out = e->patch_at_out;
    launch_patch_points(a, e->patch_at_kpts, e->patch_at_sizes, n, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, e->patch_at_out, (size_t)n * sizeof(DevPatch), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return IRMV_OK;
}

extern "C" int irmv_patch_limits(int32_t out[8])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    out[0] = kPatchW; out[1] = kPatchH; out[2] = kPatchSpanMin; out[3] = kPatchSpanMax; out[4] = kPatchRowsMax; out[5] = kPatchTopMax;
    out[6] = (int32_t)sizeof(irmv_plate_patch); out[7] = 0;
    return IRMV_OK;
}
