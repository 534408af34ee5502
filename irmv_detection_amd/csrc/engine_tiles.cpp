// Tiled search: N window slots crop out of ONE frame in one step, and the step's last node merges their result lists
// (k_tiles.hip).  Nothing here exists on an engine until its first tiled call: the merge's parameters and output records are
// allocated then, and the step plans, the op list and the graphs of ordinary steps never change.
#include "engine_internal.hpp"

static int check_tiles(const irmv_engine *e, int first, int count, const char *who)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->window) return fail(IRMV_ERR_ARG, std::string(who) + ": the engine has no window (win_width, win_height)");
    if (count < 1 || count > IRMV_MAX_TILES) return fail(IRMV_ERR_ARG, std::string(who) + ": count must be 1..IRMV_MAX_TILES");
    TRY(check_range(e, first, count));
    for (int s = first; s < first + count; s++)
        if (e->slot_view[s] != IRMV_VIEW_WINDOW)
            return fail(IRMV_ERR_ARG, std::string(who) + ": slot " + std::to_string(s) + " is in the frame view; tiles are windows (irmv_engine_set_view)");
    return IRMV_OK;
}

// The merge's device state, made by the first tiled call: the parameter pair, and per first slot the output record and its
// pinned twin.
static int ensure_tiles(irmv_engine *e, int first, irmv_engine::TileMerge **out)
{
    if (!e->tile_params_dev) {
        if (!tile_merge_prepare()) return fail(IRMV_ERR_HIP, "tile merge kernel: LDS request refused");
        TileMergeParams *p = nullptr;
        TRY(dev_alloc(e, (void **)&p, sizeof(TileMergeParams), "tile_params", mem_const(MEM_F32)));   // two floats, written by the host alone
        HIP_TRY(hipMemcpy(p, &e->tile_params, sizeof e->tile_params, hipMemcpyHostToDevice));
        e->tile_params_dev = p;
    }
    irmv_engine::TileMerge &tm = e->tile_merges[first];
    if (!tm.out_dev) {
        TileOut *d = nullptr;
        // TileOut: tile_merge_kernel writes n_kept, n_in and rec[0 .. n_kept) and reads none of it; the host indexes the slots'
        // records by rec (tile < count, index < max_det) up to n_kept.  The smallest tiled step has one tile, so zero is the
        // only word valid in every one of these uses.
        TRY(dev_alloc(e, (void **)&d, sizeof(TileOut), "tile_out." + std::to_string(first), mem_scratch_index(0u)));
        HIP_TRY(hipMemset(d, 0, sizeof(TileOut)));
        if (!tm.out_host) {
            HIP_TRY(hipHostMalloc((void **)&tm.out_host, sizeof(TileOut), hipHostMallocDefault));
            memset(tm.out_host, 0, sizeof(TileOut));
        }
        tm.out_dev = d;
    }
    *out = &tm;
    return IRMV_OK;
}

TileArgs irmv::tile_args(const irmv_engine *e, int first, int count)
{
    TileArgs a{};
    a.dets = e->dets.dev; a.fout = e->fout.dev; a.win = e->win_dev;
    a.params = e->tile_params_dev;
    a.out = e->tile_merges.at(first).out_dev;
    a.first = first; a.count = count; a.max_det = e->cfg.max_det;
    a.full_w = e->full_w; a.full_h = e->full_h; a.win_w = e->cfg.src_width; a.win_h = e->cfg.src_height; a.rotate180 = e->cfg.rotate180;
    return a;
}

// One tiled step: [upload of frame_slot's frame] -> ONE hipGraph {[demosaic of that frame] -> crop of every slot's window out
// of it -> the slots' ordinary step -> merge} -> D2H of the slots' records and of the merged list, on compute stream 0.  It is
// the slot group (first, count), submitted by the path every step takes (engine_step.cpp submit_group).
extern "C" int irmv_engine_submit_tiles(irmv_engine *e, int frame_slot, int first, int count, uint32_t flags)
{
    TRY(check_tiles(e, first, count, "irmv_engine_submit_tiles"));
    if (frame_slot < 0 || frame_slot >= e->cfg.num_slots) return fail(IRMV_ERR_ARG, "irmv_engine_submit_tiles: frame_slot out of range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    irmv_engine::TileMerge *tm;
    TRY(ensure_tiles(e, first, &tm));
    TRY(submit_group(e, first, count, flags, e->stream, frame_slot));
    tm->count = count;
    tm->valid = true;
    return IRMV_OK;
}

extern "C" int irmv_engine_merge_tiles(irmv_engine *e, int first, int count)
{
    TRY(check_tiles(e, first, count, "irmv_engine_merge_tiles"));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    irmv_engine::TileMerge *tm;
    TRY(ensure_tiles(e, first, &tm));
    if (e->zero_copy_results) {   // the slots' current records are the pinned ones: bring them to the device records the kernel reads
        TRY(e->dets.copy(first, count, hipMemcpyHostToDevice, e->stream));
        TRY(e->fout.copy(first, count, hipMemcpyHostToDevice, e->stream));
    }
    launch_tile_merge(tile_args(e, first, count), e->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tm->out_host, tm->out_dev, sizeof(TileOut), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    note_submit_windows(e, first, count);   // the merge took the corners as they are now: the slots' records are read in them from here on
    tm->count = count;
    tm->valid = true;
    return IRMV_OK;
}

extern "C" int irmv_engine_tile_results(irmv_engine *e, int first, irmv_tile_det *out, int cap, int *n, int *n_in)
{
    TRY(check_range(e, first, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    auto it = e->tile_merges.find(first);
    if (it == e->tile_merges.end() || !it->second.valid) return fail(IRMV_ERR_ARG, "irmv_engine_tile_results: no tiled step or merge has run with this first slot");
    const irmv_engine::TileMerge &tm = it->second;
    const TileOut &to = *tm.out_host;
    const int k = std::min(std::min(std::max(to.n_kept, 0), e->cfg.max_det), cap);
    for (int i = 0; i < k; i++) {
        const int t = std::min(std::max(to.rec[i][0], 0), tm.count - 1), idx = std::min(std::max(to.rec[i][1], 0), e->cfg.max_det - 1);
        slot_det(e, first + t, idx, out[i].det);
        out[i].tile = t; out[i].index = idx; out[i].cut = to.rec[i][2]; out[i].reserved = 0;
    }
    *n = k;
    if (n_in) *n_in = to.n_in;
    return IRMV_OK;
}

extern "C" int irmv_engine_set_tile_merge(irmv_engine *e, float ios_thr, float edge_margin)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!(ios_thr > 0.f && ios_thr <= 1.f)) return fail(IRMV_ERR_ARG, "irmv_engine_set_tile_merge: ios_thr must be in (0, 1]");
    if (!(edge_margin >= 0.f)) return fail(IRMV_ERR_ARG, "irmv_engine_set_tile_merge: edge_margin must be >= 0");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no merge in flight reads the pair
    e->tile_params = TileMergeParams{ios_thr, edge_margin};
    if (e->tile_params_dev) HIP_TRY(hipMemcpy(e->tile_params_dev, &e->tile_params, sizeof e->tile_params, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_get_tile_merge(const irmv_engine *e, float *ios_thr, float *edge_margin)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (ios_thr) *ios_thr = e->tile_params.ios_thr;
    if (edge_margin) *edge_margin = e->tile_params.edge_margin;
    return IRMV_OK;
}
