// What a step launches: the Detect finals' fusion as the tuner left it, the sparse head's reordering, the launch list of
// each step kind, and the ops a feature appends to it.
#include "engine_internal.hpp"

// a class-branch conv that carries its final 1x1: with emit_scan, its epilogue appends the level's scan candidates
static bool is_cls_final_carrier(const Op &op) { return op.fuse_next >= 0 && op.level >= 0 && op.layer.rfind("model.22.cv3.", 0) == 0; }

// A 3x3 conv carries its branch's final 1x1 only if BOTH of its tile choices can (LDS family, nt = 4); then the 1x1
// op drops out of the step and the tensor between the two is no longer written.
void irmv::finalize_head_fusion(irmv_engine *e)
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
    e->emit_scan = e->sw.split_scan && fused == 3 && e->sw.emit_scan;
    e->sparse_head = e->emit_scan && e->cand_bits && e->sw.sparse_head;
    e->sparse_branch = e->sparse_head && e->sw.sparse_branch;
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
//
// Candidate gather (box_gathers): a level's OP_BOXG launch stands for its first conv and its carrier; it moves behind the last
// class carrier like the carriers it replaces, and the plan's first one runs cand_list_kernel in front of itself.
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
    // Keypoint branch in the gather: a level's gather launch visits exactly the anchors whose keypoint rows the sparse OP_KPT3
    // launch would store, with the first conv's B fragments in its hands, so it computes that branch too (a fourth wave per
    // group, k_boxg.hip) and the step drops the OP_KPT3 launch.  IRMV_GATHER_KPT=0 keeps both launches; so does IRMV_KPT3=1 set
    // explicitly, which asks for kpt3_kernel by name.
    std::vector<char> rides(plan.size(), 0);
    if (e->sw.gather_kpt && !e->sw.kpt3_named)
        for (size_t i = 0; i < plan.size(); i++) {
            const Op &ko = e->ops[plan[i].op];
            if (ko.kind != OP_KPT3 || ko.level < 0 || ko.level >= 3 || !lvl_cls[ko.level] || (int)i <= last_cls) continue;
            for (size_t j = 0; j < plan.size() && !rides[i]; j++) {
                const Op &go = e->ops[plan[j].op];
                if (go.kind != OP_BOXG || go.level != ko.level) continue;
                const Op &k0 = e->ops[ko.sub[0]], &g0 = e->ops[go.sub[0]];
                if (k0.s0.t != g0.s0.t || k0.s0.coff != g0.s0.coff || k0.cin != g0.cin || ko.Hin != go.Hin || ko.Win != go.Win) continue;
                plan[j].kpt = plan[i].op;
                rides[i] = 1;
            }
        }
    std::vector<Launch> out, moved;
    bool listed = false;
    for (size_t i = 0; i < plan.size(); i++) {
        if (rides[i]) continue;   // (behind the last class carrier: nothing below is due at this index)
        Launch &l = plan[i];
        Op &op = e->ops[l.op];
        const bool boxg = op.kind == OP_BOXG;
        if (boxg) {
            l.sparse = true;
            l.cand_list = !listed;
            listed = true;
        }
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
        if ((box || first_conv[i] || boxg) && (int)i < last_cls) moved.push_back(l); else out.push_back(l);
        if ((int)i == last_cls) { out.insert(out.end(), moved.begin(), moved.end()); moved.clear(); }
    }
    plan.swap(out);
}

// Does a step (of one slot: `one`) run the box branch of OP_BOXG op g as that launch, in place of the layers it covers?  Wherever
// the sparse branch holds and the level's convs are launches of their own behind a class carrier of their own: not in a grouped
// head launch.  IRMV_SPARSE_GATHER=0 keeps the tile-gated layer launches, and so does IRMV_FORCE_WRES, which asks for the
// resident-weight kernels on every eligible layer by name.
static bool box_gathers(const irmv_engine *e, const Op &g, bool one)
{
    if (!e->sparse_branch || !e->sw.sparse_gather || e->sw.tune.has_wres || !e->boxg_list) return false;
    const Op &o0 = e->ops[g.sub[0]], &o1 = e->ops[g.sub[1]];
    if (o1.fuse_next != g.sub[2]) return false;   // (the carrier's tile choice dropped the final: the branch runs as layers)
    bool grouped = o0.group >= 0 || o1.group >= 0;
    for (const Op &op : e->ops)
        if (is_cls_final_carrier(op) && op.level == g.level) grouped = grouped || op.group >= 0;
    return !(one && grouped);
}

// ---- ops a feature appends to the steps ---------------------------------------------------
// The op kinds that are not part of the network's op list: a feature appends one to e->ops at its first enable (append_op).
// build_step_plans skips them in its loop and places their launches behind it, in this order.
static constexpr OpKind kAppendedOps[] = {OP_METER, OP_YAW, OP_POSECOV, OP_PATCH, OP_NUMBER};
static bool is_appended(OpKind k) { return std::find(std::begin(kAppendedOps), std::end(kAppendedOps), k) != std::end(kAppendedOps); }

// Everything that differs between them, decided here and nowhere else:
//   index    where the engine keeps the op's index in e->ops (-1: never enabled)
//   anchor   the launch stands directly behind the plan's last op of one of these kinds
//   records  a side-record op: run_post's plan launches it too (the meter: BATCH and ONE steps only)
//   bytes    irmv_engine_profile's per-frame figure of the launch in view v
struct AppendedOp { int *index; const char *name; std::vector<OpKind> anchor; bool records; double bytes; };
static AppendedOp appended_op(irmv_engine *e, const View &v, OpKind kind)
{
    const double md = (double)e->cfg.max_det;
    switch (kind) {
    // behind whatever produces the view's frame -- the demosaic, the crop, both at the head of the plan -- or first; it reads at
    // most the VIEW domain at step 1 on the whole view
    case OP_METER: return {&e->meter_op, "frame_meter", {OP_DEMOSAIC, OP_CROP}, false, (double)v.frame_bytes};
    // the constrained pose and the plate patches: behind the last kernel that writes the DevDet records -- the NMS, or the light
    // extraction of a classical or refined engine
    case OP_YAW: return {&e->yaw_op, "yaw_solve", {OP_NMS, OP_LIGHT}, true, md * (sizeof(DevDet) + sizeof(DevYaw))};
    // the pose uncertainty reads the yaw launch's records: behind it where the plan has one (a yaw op enabled later goes
    // directly behind the NMS, in front of it), else where the yaw launch would stand.  The patches go behind it where there is
    // one; an engine without it has no OP_POSECOV launch and the patches stand where they always did.  One order is left in
    // which the patches come first: yaw enabled, then the patches (nms, patch, yaw), then this op behind the yaw launch --
    // what it reads decides, and nothing reads across the patches.
    case OP_POSECOV: return {&e->posecov_op, "pose_cov", {OP_NMS, OP_LIGHT, OP_YAW}, true, md * (sizeof(DevDet) + sizeof(DevYaw) + sizeof(DevPoseCov))};
    case OP_PATCH: return {&e->patch_op, "plate_patch", {OP_NMS, OP_LIGHT, OP_POSECOV}, true, md * (sizeof(DevDet) + sizeof(DevPatch))};
    // the plate numbers: directly behind the patch launch whose records they read (a plan reads nms, patch, number, yaw); the
    // weights are read once per launch's detection and stay in L2
    case OP_NUMBER: return {&e->number_op, "plate_number", {OP_PATCH}, true, md * (sizeof(DevPatch) + sizeof(DevNumber)) + (double)kNumWeightHalves * sizeof(half_t)};
    default: return {nullptr, "", {}, false, 0.0};
    }
}

// The launch of appended op `kind` in the plans of view v, if the engine has the op.  It goes DIRECTLY behind its anchor: in
// front of the launches placed there before it.
static void place_appended(irmv_engine *e, View &v, OpKind kind)
{
    const AppendedOp a = appended_op(e, v, kind);
    if (!a.index || *a.index < 0) return;
    for (int k : {(int)STEP_BATCH, (int)STEP_ONE, (int)STEP_POST}) {
        if (k == STEP_POST && !a.records) continue;
        std::vector<Launch> &plan = v.plans[k];
        size_t at = a.records ? plan.size() : 0;
        for (size_t i = 0; i < plan.size(); i++)
            if (std::find(a.anchor.begin(), a.anchor.end(), e->ops[plan[i].op].kind) != a.anchor.end()) at = i + 1;
        Launch l; l.op = *a.index;
        l.name = l.layer = a.name;
        l.bytes = a.bytes;
        plan.insert(plan.begin() + at, l);
    }
}

// A feature's first enable (set_metering with options, set_yaw_solve, set_patches): the op, appended to e->ops, and its launch
// in the plans of every view built so far (a view built later gets it from build_step_plans).  Nothing of the engine is in flight.
void irmv::append_op(irmv_engine *e, OpKind kind)
{
    const AppendedOp a = appended_op(e, e->views[0], kind);
    Op op; op.kind = kind; op.layer = a.name; snprintf(op.kname, sizeof op.kname, "%s", a.name);
    e->ops.push_back(op);
    *a.index = (int)e->ops.size() - 1;
    for (View &v : e->views)
        if (v.built) place_appended(e, v, kind);
}

// The one place that decides which ops of e->ops a step of each kind launches in view v, and how.  The views differ in front
// of model.1's output only: whether the window is cut out first, and whether the front runs fused or as its three layers.
void irmv::build_step_plans(irmv_engine *e, View &v)
{
    auto is_front_layer = [&](int i) { return i == e->front_ops[0] || i == e->front_ops[1] || i == e->front_ops[2]; };
    for (int k = STEP_BATCH; k <= STEP_POST; k++) {
        v.plans[k].clear();
        const bool one = k == STEP_ONE, mat = k == STEP_MATERIALIZE, post = k == STEP_POST, step = !mat && !post;
        auto emits = [&](const Op &op) { return step && e->emit_scan && is_cls_final_carrier(op); };
        for (int i = 0; i < (int)e->ops.size(); i++) {
            const Op &op = e->ops[i];
            if (op.kind == OP_FRONT) continue;   // (launched where model.1.conv stands, below)
            if (is_appended(op.kind)) continue;   // (placed behind the loop)
            if (op.kind == OP_CROP && !v.crop) continue;
            const bool away = is_front_layer(i) ? v.fused_front : op.fused_away;   // the layers a fused kernel covers in this view
            if (post && op.kind != OP_NMS && op.kind != OP_LIGHT && op.kind != OP_SCAN) continue;
            if (op.kind == OP_SCAN && e->emit_scan && !post) continue;   // the class-branch convs have already filled the key lists
            const bool grouped = one && op.kind == OP_CONV && op.group >= 0;
            if (grouped && e->head_groups[op.group].members[0] != i) continue;   // rides in its group's launch
            // single-frame steps: the 64-channel Bottlenecks ride in their OP_BNECK launch; every other kind runs the layers
            const bool bneck = one && e->sw.bneck64;
            if (op.kind == OP_BNECK ? !bneck : (op.bneck >= 0 && bneck)) continue;
            // every step runs a level's keypoint branch as its OP_KPT3 launch (where the engine has one)
            if (op.kind == OP_KPT3 ? !step : (op.kpt3 >= 0 && step)) continue;
            // ... and a level's box branch as its OP_BOXG launch where the step gathers (box_gathers); the first conv's tensor is
            // then one no step writes: lazy, and dense again after the read-back step (Op::gated_first)
            if (op.kind == OP_BOXG ? !(step && box_gathers(e, op, one)) : (op.boxg >= 0 && step && box_gathers(e, e->ops[op.boxg], one))) continue;
            if (op.kind == OP_BOXG) {
                Op &o0 = e->ops[op.sub[0]];
                o0.gated_first = true;
                e->lazy_tensors.insert(e->tensors[o0.out_t].name);
            }
            // a step skips the layers a fused kernel covers; a read-back runs only those (and the unfused form of a conv that
            // normally carries a 1x1 in its epilogue)
            // (... and a box branch's first conv that the steps -- their plans are built first -- run behind the tile gate)
            const bool skip = mat ? !(away || op.fuse_next >= 0 || op.gated_first || ((op.bneck >= 0 || op.kpt3 >= 0) && op.kind == OP_CONV)) : away;
            if (step && v.fused_front && i == e->front_ops[2]) {   // preprocess + model.0.conv + model.1.conv as the one front launch
                const Op &fo = e->ops[e->front_op];
                Launch f; f.op = e->front_op;
                f.layer = fo.layer; f.name = fo.kname;
                f.flops = fo.flops;
                f.bytes = fo.bytes + ((double)v.frame_bytes - (double)e->frame_bytes);   // (the op counts view 0's frame)
                v.plans[k].push_back(f);
            }
            if (skip) continue;
            Launch l; l.op = i;
            // every kernel is idempotent and can be repeated inside its profile bracket -- except the light extraction and, with
            // the split scan, the scan / NMS pair (the scan appends to the frame's candidate list, the NMS kernel consumes and resets it)
            l.once = op.kind == OP_LIGHT || (e->sw.split_scan && (op.kind == OP_SCAN || op.kind == OP_NMS));
            l.keys_only = op.kind == OP_NMS && ((e->emit_scan && !post) || (post && e->sw.post_keys_only));
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
                if (op.kind == OP_PRE) l.bytes += (double)v.frame_bytes - (double)e->frame_bytes;   // (the op counts view 0's frame)
            }
            v.plans[k].push_back(l);
        }
        if (step && e->sparse_head) sparse_head_plan(e, v.plans[k]);
    }
    for (OpKind kind : kAppendedOps) place_appended(e, v, kind);
}
