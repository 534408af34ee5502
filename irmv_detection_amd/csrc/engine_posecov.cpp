// Pose uncertainty (include/irmv_hip.h, "pose uncertainty"; k_posecov.hip): the argument checks, the option table the kernel
// reads, the switch that puts the op into the engine's steps, the step's launch, the records' way to the caller, and the
// stand-alone call on an irmv_pnp.  This file is compiled with -ffp-contract=off: the stand-alone call normalises its up
// vector here, in the order irmv_detection_amd/pose_cov.py states.
#include "engine_internal.hpp"

static_assert(sizeof(irmv_pose_cov) == 288, "irmv_pose_cov is 288 bytes");
static_assert(sizeof(DevPoseCov) == sizeof(irmv_pose_cov) && offsetof(DevPoseCov, chi2) == offsetof(irmv_pose_cov, chi2) &&
                  offsetof(DevPoseCov, yaw_cov) == offsetof(irmv_pose_cov, yaw_cov) && offsetof(DevPoseCov, sigma_yaw) == offsetof(irmv_pose_cov, sigma_yaw) &&
                  offsetof(DevPoseCov, state) == offsetof(irmv_pose_cov, state) && offsetof(DevPoseCov, yaw_state) == offsetof(irmv_pose_cov, yaw_state),
              "DevPoseCov is irmv_pose_cov");
static_assert(sizeof(irmv_pose_cov_opts) == 16, "irmv_pose_cov_opts is 16 bytes");

void irmv::pose_cov_opts_defaults(irmv_pose_cov_opts *o)
{
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->enable = 0;
    o->sigma_px = 1.0;
}

// Host only; NaN fails every comparison
static int check_sigma_px(double s)
{
    if (!(s > 0.0 && s <= 64.0)) return fail(IRMV_ERR_ARG, "pose cov: sigma_px must be in (0, 64]");
    return IRMV_OK;
}

static int check_pose_cov_opts(const irmv_pose_cov_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "pose cov: opts is null");
    if (o->struct_size != sizeof(irmv_pose_cov_opts)) return fail(IRMV_ERR_ARG, "pose cov: opts.struct_size is not sizeof(irmv_pose_cov_opts)");
    if (o->enable != 0 && o->enable != 1) return fail(IRMV_ERR_ARG, "pose cov: enable must be 0 or 1");
    return check_sigma_px(o->sigma_px);
}

// e->posecov_opts -> the table.  The caller has made sure that no step in flight reads it.
static int write_pose_cov_table(irmv_engine *e)
{
    PoseCovTable t{};
    t.enable = e->posecov_opts.enable; t.sigma_px = e->posecov_opts.sigma_px;
    HIP_TRY(hipMemcpy(e->posecov_table_dev, &t, sizeof t, hipMemcpyHostToDevice));
    return IRMV_OK;
}

// The first irmv_engine_set_pose_cov: the records (device and pinned, zeroed), the table, the op and the one re-capture -- no
// captured step holds the node.  Nothing of the engine is in flight.
static int enable_pose_cov(irmv_engine *e)
{
    const size_t n = (size_t)e->cfg.num_slots * e->cfg.max_det;
    // DevPoseCov: doubles and int32 flags that only the host reads; pose_cov_kernel writes the records of [0, num_dets) where
    // it is enabled, no kernel reads one
    TRY(dev_alloc(e, (void **)&e->posecov.dev, n * sizeof(DevPoseCov), "posecov_dev", mem_scratch(MEM_F64)));
    TRY(e->posecov.pin(e, e->cfg.num_slots, e->cfg.max_det, "pinned posecov_host"));
    // a host-written table, read when the kernel runs
    TRY(dev_alloc(e, (void **)&e->posecov_table_dev, sizeof(PoseCovTable), "posecov_table", mem_const(MEM_F64)));
    append_op(e, OP_POSECOV);
    drop_graphs(e, false);   // (run_post's graphs too: the op stands behind their NMS)
    return IRMV_OK;
}

extern "C" int irmv_engine_set_pose_cov(irmv_engine *e, const irmv_pose_cov_opts *o)
{
    TRY(check_pose_cov_opts(o));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the table, no graph is running
    if (e->posecov_op < 0) TRY(enable_pose_cov(e));
    if (!o->enable) TRY(e->posecov.zero(e->cfg.num_slots));   // nothing writes the records from here on: none of an earlier step is left for a later enable to show
    e->posecov_opts = *o;
    return write_pose_cov_table(e);
}

extern "C" int irmv_engine_get_pose_cov(const irmv_engine *e, irmv_pose_cov_opts *o)
{
    if (!e || !o) return fail(IRMV_ERR_ARG, "engine / opts is null");
    *o = e->posecov_opts;
    return IRMV_OK;
}

// A step's covariances: they read the records of pa (where the step's NMS or light extraction wrote them) and, on an engine
// that solves yaws, the records the yaw launch in front has written, and go where the DevDet records go (Records::step_at).
void irmv::launch_posecov(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st)
{
    PoseCovArgs a{};
    a.dets = pa.dets; a.max_det = e->cfg.max_det;
    a.num_dets = reinterpret_cast<const int *>(pa.fout);
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.pnp = pa.pnp; a.first = s.first; a.pnp_stride = pa.pnp_stride;
    a.table = e->posecov_table_dev;
    if (e->yaw_op >= 0) { a.yaw = e->yaw.step_at(e, s); a.basis = e->yaw_basis_dev; }
    a.out = e->posecov.step_at(e, s);
    launch_pose_cov(a, s.count, st);
}

extern "C" int irmv_engine_pose_covs(irmv_engine *e, int slot, irmv_pose_cov *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (e->posecov_op < 0) return fail(IRMV_ERR_ARG, "irmv_engine_pose_covs: irmv_engine_set_pose_cov has not been called on this engine");
    // (disabled: the kernel returns at once and set_pose_cov has zeroed the records, so they stay all zero until the first
    // step after the next enable)
    return e->posecov.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_pnp_pose_cov(irmv_pnp *p, const float *img_pts, int n, int armor_size, const double *rvec, const double *tvec,
                                 const double up[3], double sigma_px, irmv_pose_cov *out)
{
    // (the values first, as the engine's call: a refused one never reaches the solver)
    if (!img_pts || !rvec || !tvec || !out || n < 0) return fail(IRMV_ERR_ARG, "null argument");
    if (armor_size != IRMV_ARMOR_SMALL && armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    TRY(check_sigma_px(sigma_px));
    PoseCovRule r{};
    r.sigma_px = sigma_px;
    if (up) {
        const double len = std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
        if (!(len > 0.0 && len < INFINITY)) return fail(IRMV_ERR_ARG, "irmv_pnp_pose_cov: up must be finite and non-zero");
        for (int i = 0; i < 3; i++) r.u[i] = up[i] / len;
        r.has_up = 1;
    }
    if (!p) return fail(IRMV_ERR_ARG, "irmv_pnp_pose_cov: solver is null");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(p->device));
    TRY(pnp_reserve(p, n));
    std::vector<double> poses((size_t)n * 6);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) { poses[(size_t)i * 6 + k] = rvec[(size_t)i * 3 + k]; poses[(size_t)i * 6 + 3 + k] = tvec[(size_t)i * 3 + k]; }
    HIP_TRY(hipMemcpyAsync(p->pts, img_pts, (size_t)n * 32, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->cov_poses, poses.data(), poses.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
    launch_pose_cov_points(p->c, p->pts, p->cov_poses, n, armor_size, r, p->cov, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, p->cov, (size_t)n * sizeof(DevPoseCov), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));   // (poses outlives the copy that reads it)
    return IRMV_OK;
}
