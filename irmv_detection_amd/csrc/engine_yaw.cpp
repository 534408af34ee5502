// Constrained pose (include/irmv_hip.h, "constrained pose"; k_yaw.hip): the argument checks, the two tables the kernel reads
// and everything that rewrites them, the switch that puts the op into the engine's steps, the step's launch, the records'
// way to the caller, and the stand-alone call on an irmv_pnp.  This file is compiled with -ffp-contract=off: the basis and c
// are computed here, in the order irmv_detection_amd/yaw_solve.py states, and the device never normalises a vector.
#include "engine_internal.hpp"

static_assert(sizeof(DevYaw) == sizeof(irmv_yaw_pose) && offsetof(DevYaw, tau) == offsetof(irmv_yaw_pose, tau) &&
                  offsetof(DevYaw, state) == offsetof(irmv_yaw_pose, state) && offsetof(DevYaw, lane) == offsetof(irmv_yaw_pose, lane) &&
                  sizeof(DevYaw) % 8 == 0,
              "DevYaw is irmv_yaw_pose");
static_assert(kYawRoundsMax == 6, "irmv_yaw_pose.lane has six entries");

void irmv::yaw_opts_defaults(irmv_yaw_opts *o)
{
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->enable = 0;
    o->rounds = 4;
    o->tau_max = 1.0;
    o->horizon_min = 1e-4;
}

// Host only; NaN fails every comparison
static int check_yaw_opts(const irmv_yaw_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "yaw solve: opts is null");
    if (o->struct_size != sizeof(irmv_yaw_opts)) return fail(IRMV_ERR_ARG, "yaw solve: opts.struct_size is not sizeof(irmv_yaw_opts)");
    if (o->enable != 0 && o->enable != 1) return fail(IRMV_ERR_ARG, "yaw solve: enable must be 0 or 1");
    if (o->rounds < 1 || o->rounds > kYawRoundsMax) return fail(IRMV_ERR_ARG, "yaw solve: rounds must be 1 .. 6");
    if (o->reserved != 0) return fail(IRMV_ERR_ARG, "yaw solve: reserved must be 0");
    if (!(o->tau_max > 0.0 && o->tau_max <= 4.0)) return fail(IRMV_ERR_ARG, "yaw solve: tau_max must be in (0, 4]");
    if (!(o->horizon_min > 0.0 && o->horizon_min < 1.0)) return fail(IRMV_ERR_ARG, "yaw solve: horizon_min must be in (0, 1)");
    return IRMV_OK;
}

// The slot's basis from its unit up vector: g = e_z - (e_z . u) u, h1 = g / |g|, h2 = u x h1 (yaw_solve.py basis())
static YawBasis yaw_basis(const double *u, double horizon_min)
{
    YawBasis b{};
    for (int i = 0; i < 3; i++) b.u[i] = u[i];
    const double ezu = u[2];
    const double g[3] = {0.0 - ezu * u[0], 0.0 - ezu * u[1], 1.0 - ezu * u[2]};
    const double g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    if (!(g2 >= horizon_min)) return b;   // (negated: a NaN has no basis either)
    const double len = std::sqrt(g2);
    for (int i = 0; i < 3; i++) b.h1[i] = g[i] / len;
    b.h2[0] = u[1] * b.h1[2] - u[2] * b.h1[1];
    b.h2[1] = u[2] * b.h1[0] - u[0] * b.h1[2];
    b.h2[2] = u[0] * b.h1[1] - u[1] * b.h1[0];
    b.ok = 1;
    return b;
}

static double yaw_c(double s) { return std::sqrt(1.0 - s * s); }   // 0 (|s| = 1) or NaN: the class has no basis

// e->yaw_opts, e->pose_prior and e->up -> the table and the bases (slot >= 0: that slot's basis alone).  The caller has made
// sure that no step in flight reads what is rewritten.
int irmv::write_yaw_tables(irmv_engine *e, int slot)
{
    if (e->yaw_op < 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int S = e->cfg.num_slots;
    if (slot < 0) {
        YawTable t{};
        t.enable = e->yaw_opts.enable; t.rounds = e->yaw_opts.rounds; t.tau_max = e->yaw_opts.tau_max;
        for (int c = 0; c < kMaxClasses; c++) { t.s[c] = e->pose_prior.normal_up[c]; t.c[c] = yaw_c(t.s[c]); }
        HIP_TRY(hipMemcpy(e->yaw_table_dev, &t, sizeof t, hipMemcpyHostToDevice));
    }
    std::vector<YawBasis> b;
    const int s0 = slot < 0 ? 0 : slot, s1 = slot < 0 ? S : slot + 1;
    for (int s = s0; s < s1; s++) b.push_back(yaw_basis(e->up.data() + 3 * s, e->yaw_opts.horizon_min));
    HIP_TRY(hipMemcpy(e->yaw_basis_dev + s0, b.data(), b.size() * sizeof(YawBasis), hipMemcpyHostToDevice));
    return IRMV_OK;
}

// The first irmv_engine_set_yaw_solve: the records (device and pinned, zeroed), the two tables, the op and the one re-capture --
// no captured step holds the yaw node.  Nothing of the engine is in flight.
static int enable_yaw(irmv_engine *e)
{
    const size_t n = (size_t)e->cfg.num_slots * e->cfg.max_det;
    // DevYaw: doubles and int32 flags that only the host reads; yaw_solve_kernel writes the records of [0, num_dets) where it
    // is enabled, no kernel reads one
    TRY(dev_alloc(e, (void **)&e->yaw.dev, n * sizeof(DevYaw), "yaw_dev", mem_scratch(MEM_F64)));
    TRY(e->yaw.pin(e, e->cfg.num_slots, e->cfg.max_det, "pinned yaw_host"));
    // host-written tables, read when the kernel runs
    TRY(dev_alloc(e, (void **)&e->yaw_table_dev, sizeof(YawTable), "yaw_table", mem_const(MEM_F64)));
    TRY(dev_alloc(e, (void **)&e->yaw_basis_dev, (size_t)e->cfg.num_slots * sizeof(YawBasis), "yaw_basis", mem_const(MEM_F64)));
    append_op(e, OP_YAW);
    drop_graphs(e, false);   // (run_post's graphs too: the op stands behind their NMS)
    return IRMV_OK;
}

extern "C" int irmv_engine_set_yaw_solve(irmv_engine *e, const irmv_yaw_opts *o)
{
    TRY(check_yaw_opts(o));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));   // every stream of the engine: no step in flight reads the tables, no graph is running
    if (e->yaw_op < 0) TRY(enable_yaw(e));
    if (!o->enable) TRY(e->yaw.zero(e->cfg.num_slots));   // nothing writes the records from here on: none of an earlier step is left for a later enable to show
    e->yaw_opts = *o;
    return write_yaw_tables(e);
}

extern "C" int irmv_engine_get_yaw_solve(const irmv_engine *e, irmv_yaw_opts *o)
{
    if (!e || !o) return fail(IRMV_ERR_ARG, "engine / opts is null");
    *o = e->yaw_opts;
    return IRMV_OK;
}

// A step's constrained poses: they read the records of pa (where the step's NMS or light extraction wrote them) and go where
// the DevDet records go (Records::step_at).
void irmv::launch_yaw(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st)
{
    YawArgs a{};
    a.dets = pa.dets; a.max_det = e->cfg.max_det;
    a.num_dets = reinterpret_cast<const int *>(pa.fout);
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.pnp = pa.pnp; a.first = s.first; a.pnp_stride = pa.pnp_stride;
    a.table = e->yaw_table_dev; a.basis = e->yaw_basis_dev;
    a.out = e->yaw.step_at(e, s);
    launch_yaw_solve(a, s.count, st);
}

extern "C" int irmv_engine_yaw_poses(irmv_engine *e, int slot, irmv_yaw_pose *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (e->yaw_op < 0) return fail(IRMV_ERR_ARG, "irmv_engine_yaw_poses: irmv_engine_set_yaw_solve has not been called on this engine");
    // (disabled: the kernel returns at once and set_yaw_solve has zeroed the records, so they stay all zero until the first
    // step after the next enable)
    return e->yaw.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_pnp_solve_yaw(irmv_pnp *p, const float *img_pts, int n, int armor_size, const double up[3], double normal_up,
                                  const irmv_yaw_opts *o, irmv_yaw_pose *out)
{
    // (the values first, as the engine's call: a refused one never reaches the solver)
    if (!img_pts || !up || !out || n < 0) return fail(IRMV_ERR_ARG, "null argument");
    if (armor_size != IRMV_ARMOR_SMALL && armor_size != IRMV_ARMOR_LARGE) return fail(IRMV_ERR_ARG, "bad armor_size");
    irmv_yaw_opts oo;
    if (o) { oo = *o; if (oo.struct_size == sizeof oo) oo.enable = 1; }   // (enable is not read: only its range would be checked)
    TRY(check_yaw_opts(o ? &oo : nullptr));
    if (!(std::fabs(normal_up) <= 1.0)) return fail(IRMV_ERR_ARG, "irmv_pnp_solve_yaw: normal_up must be in [-1, 1]");
    const double len = std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
    if (!(len > 0.0 && len < INFINITY)) return fail(IRMV_ERR_ARG, "irmv_pnp_solve_yaw: up must be finite and non-zero");
    if (!p) return fail(IRMV_ERR_ARG, "irmv_pnp_solve_yaw: solver is null");
    if (n == 0) return IRMV_OK;
    const double u[3] = {up[0] / len, up[1] / len, up[2] / len};
    const YawBasis b = yaw_basis(u, o->horizon_min);
    YawRule r{};
    for (int i = 0; i < 3; i++) { r.u[i] = b.u[i]; r.h1[i] = b.h1[i]; r.h2[i] = b.h2[i]; }
    r.s = normal_up; r.c = yaw_c(normal_up); r.tau_max = o->tau_max; r.rounds = o->rounds; r.ok = b.ok;
    HIP_TRY(hipSetDevice(p->device));
    TRY(pnp_reserve(p, n));
    HIP_TRY(hipMemcpyAsync(p->pts, img_pts, (size_t)n * 32, hipMemcpyHostToDevice, p->stream));
    launch_yaw_points(p->c, p->pts, n, armor_size, r, p->yaw, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, p->yaw, (size_t)n * sizeof(DevYaw), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return IRMV_OK;
}
