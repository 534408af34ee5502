// Armor tracks (include/irmv_hip.h, "armor tracks"; k_track.hip): the option checks, the switch, the per-slot stamp and camera
// pose, the launch behind a step and its place in the submit order, the records' way to the caller, the stand-alone tracker and
// the host helper irmv_track_predict.  This file is compiled with -ffp-contract=off: irmv_track_predict runs the kernel's own
// prediction (track_math.hpp) on the host, in the order irmv_detection_amd/tracks.py states.
#include "engine_internal.hpp"
#include "track_math.hpp"

static_assert(sizeof(irmv_track_opts) == 72, "irmv_track_opts is 72 bytes");
static_assert(sizeof(irmv_det_track) == 72 && sizeof(DevDetTrack) == 72, "irmv_det_track is 72 bytes");
static_assert(sizeof(irmv_track_frame) == 40 && sizeof(DevTrackFrame) == 40, "irmv_track_frame is 40 bytes");
static_assert(sizeof(irmv_track) == 384 && sizeof(DevTrack) == 384, "irmv_track is 384 bytes");
static_assert(sizeof(irmv_track_obs) == 112 && sizeof(TrackObs) == 112, "irmv_track_obs is 112 bytes");
static_assert(kTrackClasses == IRMV_NUM_CLASSES, "the class the tracker sees is irmv_det.class_id");
static_assert(IRMV_TRACK_CAP == kTrackCap && sizeof(DevTrackSnap) == 40 + 32 * 384, "a slot's snapshot: the header, then the table");
static_assert(offsetof(DevDetTrack, d2) == offsetof(irmv_det_track, d2) && offsetof(DevDetTrack, vel) == offsetof(irmv_det_track, vel) &&
                  offsetof(DevTrackFrame, next_id) == offsetof(irmv_track_frame, next_id) && offsetof(DevTrack, det) == offsetof(irmv_track, det) &&
                  offsetof(DevTrack, stamp) == offsetof(irmv_track, stamp) && offsetof(DevTrack, x) == offsetof(irmv_track, x) &&
                  offsetof(DevTrack, P) == offsetof(irmv_track, P) && offsetof(TrackObs, tvec) == offsetof(irmv_track_obs, tvec) &&
                  offsetof(TrackObs, cov) == offsetof(irmv_track_obs, cov),
              "the device records are the ABI's");

void irmv::track_opts_defaults(irmv_track_opts *o)
{
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->enable = 0;
    o->confirm_hits = 3; o->max_misses = 5; o->match_class = 1;
    o->gate = 16.27; o->max_coast_s = 0.5; o->accel_sigma = 8.0; o->init_vel_sigma = 3.0; o->sigma_lat = 0.002; o->sigma_rng = 0.01;
}

// Host only; NaN fails every comparison
static bool positive(double v) { return v > 0.0 && v < INFINITY; }

static int check_track_opts(const irmv_track_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "tracking: opts is null");
    if (o->struct_size != sizeof(irmv_track_opts)) return fail(IRMV_ERR_ARG, "tracking: opts.struct_size is not sizeof(irmv_track_opts)");
    if (o->enable != 0 && o->enable != 1) return fail(IRMV_ERR_ARG, "tracking: enable must be 0 or 1");
    if (o->match_class != 0 && o->match_class != 1) return fail(IRMV_ERR_ARG, "tracking: match_class must be 0 or 1");
    if (o->confirm_hits < 1 || o->confirm_hits > (1 << 20)) return fail(IRMV_ERR_ARG, "tracking: confirm_hits must be in [1, 2^20]");
    if (o->max_misses < 1 || o->max_misses > (1 << 20)) return fail(IRMV_ERR_ARG, "tracking: max_misses must be in [1, 2^20]");
    if (o->reserved != 0) return fail(IRMV_ERR_ARG, "tracking: reserved must be 0");
    if (!positive(o->gate) || !positive(o->max_coast_s) || !positive(o->accel_sigma) || !positive(o->init_vel_sigma) || !positive(o->sigma_lat) ||
        !positive(o->sigma_rng))
        return fail(IRMV_ERR_ARG, "tracking: gate, max_coast_s, accel_sigma, init_vel_sigma, sigma_lat and sigma_rng must be finite and positive");
    return IRMV_OK;
}

extern "C" int irmv_track_default_opts(irmv_track_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "opts is null");
    track_opts_defaults(o);
    return IRMV_OK;
}

static TrackOpts table_of(const irmv_track_opts &o)
{
    TrackOpts t{};
    t.enable = o.enable; t.confirm_hits = o.confirm_hits; t.max_misses = o.max_misses; t.match_class = o.match_class;
    t.gate = o.gate; t.max_coast_s = o.max_coast_s; t.accel_sigma = o.accel_sigma; t.init_vel_sigma = o.init_vel_sigma;
    t.sigma_lat = o.sigma_lat; t.sigma_rng = o.sigma_rng;
    return t;
}

// The table and its stamp to "empty", the id counter kept.  The caller has made sure that nothing of the engine is in flight.
static int clear_track_table(DevTrackTable *dev, uint32_t next_id)
{
    HIP_TRY(hipMemset(dev, 0, sizeof(DevTrackTable)));
    HIP_TRY(hipMemcpy(&dev->next_id, &next_id, sizeof next_id, hipMemcpyHostToDevice));
    return IRMV_OK;
}

static int read_next_id(const DevTrackTable *dev, uint32_t *id)
{
    HIP_TRY(hipMemcpy(id, &dev->next_id, sizeof *id, hipMemcpyDeviceToHost));
    return IRMV_OK;
}

static int write_track_slot(irmv_engine *e, int slot)
{
    if (!e->track_made) return IRMV_OK;   // (the first set_tracking uploads every slot's entry)
    HIP_TRY(hipMemcpy(e->track_slots_dev + slot, &e->track_slots[slot], sizeof(TrackSlot), hipMemcpyHostToDevice));
    return IRMV_OK;
}

// The first irmv_engine_set_tracking: the two channels (device and pinned, zeroed), the carried table, the option table, the
// per-slot stamps and poses, the event.  No op, no node: nothing is re-captured.  Nothing of the engine is in flight.  Every
// step is skipped where its result exists, so a call that failed half-way is finished by the next one and registers no range
// twice.
static int enable_tracking(irmv_engine *e)
{
    const int S = e->cfg.num_slots;
    // DevDetTrack: int32 fields and doubles that only the host reads; track_kernel writes the records of [0, num_dets), no kernel reads one
    if (!e->dettrack.dev) TRY(dev_alloc(e, (void **)&e->dettrack.dev, (size_t)S * e->cfg.max_det * sizeof(DevDetTrack), "dettrack_dev", mem_scratch(MEM_F64)));
    if (!e->dettrack.host) TRY(e->dettrack.pin(e, S, e->cfg.max_det, "pinned dettrack_host"));
    // DevTrackSnap: track_kernel writes the whole record of a fed slot, no kernel reads one
    if (!e->tracks.dev) TRY(dev_alloc(e, (void **)&e->tracks.dev, (size_t)S * sizeof(DevTrackSnap), "tracks_dev", mem_scratch(MEM_F64)));
    if (!e->tracks.host) TRY(e->tracks.pin(e, S, 1, "pinned tracks_host"));
    // CARRIED, invariant: the track table as the last fed step left it (empty, stamped = 0, next_id = 1 at first).  Entry indices,
    // ids, counters: track_kernel reads `state` as a three-way flag and `det` never; nothing indexes memory by a word of it
    if (!e->track_table_dev) TRY(dev_alloc(e, (void **)&e->track_table_dev, sizeof(DevTrackTable), "track_table", mem_carried_index(0xffffffffu)));
    TRY(clear_track_table(e->track_table_dev, 1u));
    // two host-written tables, read when the kernel runs
    if (!e->track_opts_dev) TRY(dev_alloc(e, (void **)&e->track_opts_dev, sizeof(TrackOpts), "track_opts", mem_const(MEM_F64)));
    if (!e->track_slots_dev) TRY(dev_alloc(e, (void **)&e->track_slots_dev, (size_t)S * sizeof(TrackSlot), "track_slots", mem_const(MEM_F64)));
    HIP_TRY(hipMemcpy(e->track_slots_dev, e->track_slots.data(), (size_t)S * sizeof(TrackSlot), hipMemcpyHostToDevice));
    if (!e->track_event) HIP_TRY(hipEventCreateWithFlags(&e->track_event, hipEventDisableTiming));
    e->track_made = true;
    return IRMV_OK;
}

extern "C" int irmv_engine_set_tracking(irmv_engine *e, const irmv_track_opts *o)
{
    TRY(check_track_opts(o));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no track launch in flight reads the tables or writes the table
    if (!e->track_made) TRY(enable_tracking(e));
    if (!o->enable) {
        // nothing writes the records from here on, and a later enable starts from an empty table with the ids going on
        uint32_t next_id = 1;
        TRY(read_next_id(e->track_table_dev, &next_id));
        TRY(clear_track_table(e->track_table_dev, next_id));
        TRY(e->dettrack.zero(e->cfg.num_slots));
        TRY(e->tracks.zero(e->cfg.num_slots));
    }
    e->track_opts = *o;
    e->track_event_stream = nullptr;
    const TrackOpts t = table_of(*o);
    HIP_TRY(hipMemcpy(e->track_opts_dev, &t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_get_tracking(const irmv_engine *e, irmv_track_opts *o)
{
    if (!e || !o) return fail(IRMV_ERR_ARG, "engine / opts is null");
    *o = e->track_opts;
    return IRMV_OK;
}

extern "C" int irmv_engine_set_stamp(irmv_engine *e, int slot, double t)
{
    if (!trk_finite(t)) return fail(IRMV_ERR_ARG, "irmv_engine_set_stamp: the stamp must be finite");
    TRY(check_range(e, slot, 1));
    if (e->track_made) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read the slot's entry
    }
    e->track_slots[slot].stamp = t;
    return write_track_slot(e, slot);
}

extern "C" int irmv_engine_get_stamp(const irmv_engine *e, int slot, double *t)
{
    TRY(check_range(e, slot, 1));
    if (!t) return fail(IRMV_ERR_ARG, "t is null");
    *t = e->track_slots[slot].stamp;
    return IRMV_OK;
}

extern "C" int irmv_engine_set_camera_pose(irmv_engine *e, int slot, const double R_wc[9], const double t_wc[3])
{
    if (!R_wc || !t_wc) return fail(IRMV_ERR_ARG, "R_wc / t_wc is null");
    for (int i = 0; i < 9; i++)
        if (!trk_finite(R_wc[i])) return fail(IRMV_ERR_ARG, "irmv_engine_set_camera_pose: R_wc must be finite");
    for (int i = 0; i < 3; i++)
        if (!trk_finite(t_wc[i])) return fail(IRMV_ERR_ARG, "irmv_engine_set_camera_pose: t_wc must be finite");
    TRY(check_range(e, slot, 1));
    if (e->track_made) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        TRY(irmv_engine_wait_slots(e, slot, 1));   // the slot's last step has read the slot's entry
    }
    std::copy(R_wc, R_wc + 9, e->track_slots[slot].R);
    std::copy(t_wc, t_wc + 3, e->track_slots[slot].t);
    return write_track_slot(e, slot);
}

extern "C" int irmv_engine_get_camera_pose(const irmv_engine *e, int slot, double R_wc[9], double t_wc[3])
{
    TRY(check_range(e, slot, 1));
    if (!R_wc || !t_wc) return fail(IRMV_ERR_ARG, "R_wc / t_wc is null");
    std::copy(e->track_slots[slot].R, e->track_slots[slot].R + 9, R_wc);
    std::copy(e->track_slots[slot].t, e->track_slots[slot].t + 3, t_wc);
    return IRMV_OK;
}

// Behind an ordinary step's graph (or eager launches) on its stream st, in front of the results' copy-out: the table advances
// over the step's slots, in slot order.  The launches of steps on different streams are chained by ONE event, in submit order:
// the step bodies still overlap, only the track launches queue.
int irmv::track_step(irmv_engine *e, const Step &s, hipStream_t st)
{
    if (!e->track_made || !e->track_opts.enable) return IRMV_OK;
    if (e->track_event_stream && e->track_event_stream != st) HIP_TRY(hipStreamWaitEvent(st, e->track_event, 0));
    TrackArgs a{};
    a.table = e->track_table_dev; a.opts = e->track_opts_dev; a.slots = e->track_slots_dev; a.first = s.first;
    a.dets = e->dets.step_at(e, s); a.max_det = e->cfg.max_det;   // where the step's NMS or light extraction wrote them (post_args)
    a.num_dets = reinterpret_cast<const int *>(e->fout.step_at(e, s));
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    if (e->posecov_op >= 0 && e->posecov_opts.enable) a.cov = e->posecov.step_at(e, s);
    a.out_det = e->dettrack.step_at(e, s);
    a.out_snap = e->tracks.step_at(e, s);
    launch_track_update(a, s.count, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->track_event, st));
    e->track_event_stream = st;
    return IRMV_OK;
}

// A step that does not feed the tracker (a tiled step, run_post): its slots' two channels read as zero, on stream st.
// copied: copy_out_dev follows on st and brings the zeroed device records to their pinned twins; else (run_post on an engine
// with zero-copy results) the twins are zeroed through their device view.
int irmv::track_skip(irmv_engine *e, int first, int count, hipStream_t st, bool copied)
{
    if (!e->track_made || !e->track_opts.enable) return IRMV_OK;
    const size_t nd = (size_t)count * e->cfg.max_det * sizeof(DevDetTrack), ns = (size_t)count * sizeof(DevTrackSnap);
    if (copied) {
        HIP_TRY(hipMemsetAsync(e->dettrack.dev_at(first), 0, nd, st));
        HIP_TRY(hipMemsetAsync(e->tracks.dev_at(first), 0, ns, st));
    } else {
        HIP_TRY(hipMemsetAsync(e->dettrack.host_dev + (size_t)first * e->cfg.max_det, 0, nd, st));
        HIP_TRY(hipMemsetAsync(e->tracks.host_dev + first, 0, ns, st));
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_det_tracks(irmv_engine *e, int slot, irmv_det_track *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (!e->track_made) return fail(IRMV_ERR_ARG, "irmv_engine_det_tracks: irmv_engine_set_tracking has not been called on this engine");
    return e->dettrack.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_engine_tracks(irmv_engine *e, int slot, irmv_track_frame *frame, irmv_track *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (!e->track_made) return fail(IRMV_ERR_ARG, "irmv_engine_tracks: irmv_engine_set_tracking has not been called on this engine");
    const DevTrackSnap *s = e->tracks.host_at(slot);
    if (frame) memcpy(frame, &s->frame, sizeof *frame);
    const int k = std::max(0, std::min(cap, kTrackCap));
    if (k) memcpy(out, s->tracks, (size_t)k * sizeof(DevTrack));
    *n = k;
    return IRMV_OK;
}

extern "C" int irmv_engine_reset_tracks(irmv_engine *e)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->track_made) return IRMV_OK;   // (no table yet: nothing to clear)
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    uint32_t next_id = 1;
    TRY(read_next_id(e->track_table_dev, &next_id));
    return clear_track_table(e->track_table_dev, next_id);
}

extern "C" int irmv_track_limits(int32_t out[8])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    const int32_t v[8] = {kTrackCap, (int32_t)sizeof(irmv_track), (int32_t)sizeof(irmv_det_track), (int32_t)sizeof(irmv_track_frame),
                          (int32_t)sizeof(irmv_track_opts), kMaxDetCap, 0, 0};
    std::copy(v, v + 8, out);
    return IRMV_OK;
}

extern "C" int irmv_track_predict(const irmv_track *track, double t, double accel_sigma, double pos[3], double cov[9])
{
    if (!track || !pos || !cov) return fail(IRMV_ERR_ARG, "null argument");
    const double dt = t - track->stamp;
    if (track->state == IRMV_TRACK_FREE) return fail(IRMV_ERR_ARG, "irmv_track_predict: the track is free");
    if (!(dt >= 0.0 && dt < INFINITY)) return fail(IRMV_ERR_ARG, "irmv_track_predict: t must be finite and not before the track's stamp");
    if (!positive(accel_sigma)) return fail(IRMV_ERR_ARG, "irmv_track_predict: accel_sigma must be finite and positive");
    double x[6], P[36];
    std::copy(track->x, track->x + 6, x);
    std::copy(track->P, track->P + 36, P);
    trk_predict(x, P, dt, accel_sigma);
    for (int i = 0; i < 3; i++) {
        pos[i] = x[i];
        for (int j = 0; j < 3; j++) cov[3 * i + j] = P[6 * i + j];
    }
    return IRMV_OK;
}

// ---- the stand-alone tracker ----------------------------------------------------------------------------------------------
// The object owns no device memory: its table, options, pose and the call's buffers are ONE block of mapped, coherent pinned
// host memory that the kernel reads and writes through the device's view of it, as a zero-copy engine's records are.
struct TrackerBlock {
    DevTrackTable table;
    TrackOpts opts;
    TrackSlot slot;
    TrackObs obs[kMaxDetCap];
    DevDetTrack det[kMaxDetCap];
    DevTrackSnap snap;
};
struct irmv_tracker {
    int device = 0;
    hipStream_t stream = nullptr;
    TrackerBlock *host = nullptr, *dev = nullptr;
};

extern "C" void irmv_tracker_destroy(irmv_tracker *tr)
{
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) { (void)hipStreamSynchronize(tr->stream); (void)hipStreamDestroy(tr->stream); }
    if (tr->host) (void)hipHostFree(tr->host);
    delete tr;
}

extern "C" int irmv_tracker_create(int device, const irmv_track_opts *opts, irmv_tracker **out)
{
    irmv_track_opts o;
    if (opts) { TRY(check_track_opts(opts)); o = *opts; }
    else { track_opts_defaults(&o); o.enable = 1; }
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(IRMV_ERR_HIP, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    irmv_tracker *tr = new irmv_tracker;
    tr->device = device;
    int rc = IRMV_OK;
    hipError_t he = hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipHostMalloc((void **)&tr->host, sizeof(TrackerBlock), hipHostMallocMapped | hipHostMallocCoherent);
    if (he == hipSuccess) he = hipHostGetDevicePointer((void **)&tr->dev, tr->host, 0);
    if (he != hipSuccess) rc = fail(IRMV_ERR_HIP, std::string("irmv_tracker_create: ") + hipGetErrorString(he));
    if (rc) { irmv_tracker_destroy(tr); return rc; }
    memset(tr->host, 0, sizeof(TrackerBlock));
    tr->host->table.next_id = 1;
    tr->host->opts = table_of(o);
    *out = tr;
    return IRMV_OK;
}

extern "C" int irmv_tracker_reset(irmv_tracker *tr)
{
    if (!tr) return fail(IRMV_ERR_ARG, "tracker is null");
    const uint32_t next_id = tr->host->table.next_id;   // (every update has synchronised its stream)
    memset(&tr->host->table, 0, sizeof(DevTrackTable));
    tr->host->table.next_id = next_id;
    return IRMV_OK;
}

extern "C" int irmv_tracker_update(irmv_tracker *tr, double t, const double R_wc[9], const double t_wc[3], const irmv_track_obs *obs, int n,
                                   irmv_det_track *det_out, irmv_track_frame *frame, irmv_track *tracks_out)
{
    if (!tr) return fail(IRMV_ERR_ARG, "tracker is null");
    if (n < 0 || n > kMaxDetCap || (n > 0 && !obs)) return fail(IRMV_ERR_ARG, "irmv_tracker_update: n must be in [0, 256] and obs not null");
    static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
    const double *R = R_wc ? R_wc : eye, *tw = t_wc ? t_wc : zero;
    for (int i = 0; i < 9; i++)
        if (!trk_finite(R[i])) return fail(IRMV_ERR_ARG, "irmv_tracker_update: R_wc must be finite");
    for (int i = 0; i < 3; i++)
        if (!trk_finite(tw[i])) return fail(IRMV_ERR_ARG, "irmv_tracker_update: t_wc must be finite");
    HIP_TRY(hipSetDevice(tr->device));
    TrackerBlock *h = tr->host, *d = tr->dev;
    h->slot.stamp = t;
    std::copy(R, R + 9, h->slot.R);
    std::copy(tw, tw + 3, h->slot.t);
    if (n) memcpy(h->obs, obs, (size_t)n * sizeof(TrackObs));
    TrackArgs a{};
    a.table = &d->table; a.opts = &d->opts; a.slots = &d->slot; a.first = 0;
    a.max_det = kMaxDetCap;
    a.obs = d->obs; a.n_obs = n;
    a.out_det = d->det; a.out_snap = &d->snap;
    launch_track_update(a, 1, tr->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(tr->stream));
    if (det_out && n) memcpy(det_out, h->det, (size_t)n * sizeof(DevDetTrack));
    if (frame) memcpy(frame, &h->snap.frame, sizeof *frame);
    if (tracks_out) memcpy(tracks_out, h->snap.tracks, sizeof h->snap.tracks);
    return IRMV_OK;
}
