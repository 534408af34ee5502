// Running a step: the kernel arguments of every op kind, the one launcher, frame copies, the record channels (where a step's
// records go and how they reach the host), graph capture, and the submit / wait / results ABI.
#include "engine_internal.hpp"

// ---- kernel arguments: one builder per op kind, on slots [first, first + count) -----------
void irmv::fill_conv_args(const irmv_engine *e, const Op &op, int first, int count, ConvArgs &a, bool fused)
{
    a = ConvArgs{};
    auto seg = [&](const SegRef &s) {
        ConvSeg cs{nullptr, 0, 0, 0};
        if (s.t < 0 || s.C == 0) return cs;
        const Tensor &t = e->tensors[s.t];
        cs.p = static_cast<const half_t *>(t.slot(first)) + s.coff;
        cs.ld = t.C;
        cs.C = s.C;
        cs.shift = s.shift;
        return cs;
    };
    a.s0 = seg(op.s0);
    a.s1 = seg(op.s1);
    a.Hin = op.Hin; a.Win = op.Win; a.Hout = op.Hout; a.Wout = op.Wout;
    a.M = count * op.Hout * op.Wout;
    a.Cin = op.cin;
    a.w = op.w_packed;
    a.bias = op.bias;
    const Tensor &ot = e->tensors[op.out_t];
    a.out = static_cast<char *>(ot.slot(first)) + (size_t)op.out_coff * ot.esize();
    a.out_ld = ot.C;
    a.res = nullptr;
    a.res_ld = 0;
    if (op.res_t >= 0) {
        const Tensor &rt = e->tensors[op.res_t];
        a.res = static_cast<const half_t *>(rt.slot(first)) + op.res_coff;
        a.res_ld = rt.C;
    }
    a.cout_pad = op.cout_pad;
    a.ksteps = op.ksteps;
    a.pair = op.pair ? 1 : 0;
    a.w2 = nullptr; a.bias2 = nullptr; a.out2 = nullptr; a.out2_ld = 0; a.n2 = 0;
    if (fused && op.fuse_next >= 0) {
        const Op &o2 = e->ops[op.fuse_next];
        const Tensor &t2 = e->tensors[o2.out_t];
        a.w2 = op.cfg.cin16 ? o2.w_k16 : o2.w_packed;
        a.bias2 = o2.bias;
        a.out2 = static_cast<float *>(t2.slot(first)) + o2.out_coff;
        a.out2_ld = t2.C;
        a.n2 = o2.cout_pad / 16;
    }
    if (op.w_k16) a.w2 = op.w_k16;   // a Cin = 16 final as its own launch (k_conv.hip conv1x1_k16_f32_kernel)
}

// All slots of a step are in one view: *view = that of [first, first + count), or IRMV_ERR_ARG naming the first two that differ.
int irmv::slots_view(const irmv_engine *e, int first, int count, int *view)
{
    if (view) *view = e->slot_view[first];
    for (int s = first + 1; s < first + count; s++)
        if (e->slot_view[s] != e->slot_view[first])
            return fail(IRMV_ERR_ARG, "slots " + std::to_string(first) + " and " + std::to_string(s) + " are in different views (irmv_engine_set_view): one step runs one view");
    return IRMV_OK;
}

LightArgs irmv::light_args(const irmv_engine *e, const View &v, int first)
{
    LightArgs a{};
    const irmv_engine_cfg &c = e->cfg;
    a.frames = v.frames + (size_t)first * v.frame_bytes;
    a.frame_bytes = v.frame_bytes;
    a.cols = v.src_w; a.rows = v.src_h; a.rotate180 = c.rotate180;
    a.dets = e->dets.dev_at(first);
    a.max_det = c.max_det;
    a.num_dets = reinterpret_cast<const int *>(e->fout.dev_at(first));
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.n_boxes = 0;
    a.boxes = nullptr;
    a.labels = v.light_labels + (size_t)first * v.light_pool;
    a.label_pool = v.light_pool;
    a.points = e->light_points + (size_t)first * c.max_det * kLightPointsCap * 2;
    a.points_cap = kLightPointsCap;
    a.hulls = e->light_hulls + (size_t)first * c.max_det * kLightPointsCap * 4;
    a.binary_threshold = c.binary_threshold;
    a.light_min_ratio = c.light_min_ratio; a.light_max_ratio = c.light_max_ratio; a.light_max_angle = c.light_max_angle;
    a.min_small_cd = c.armor_min_small_center_distance; a.max_small_cd = c.armor_max_small_center_distance;
    a.min_large_cd = c.armor_min_large_center_distance; a.max_large_cd = c.armor_max_large_center_distance;
    a.pnp = e->pnp_dev;
    a.first = first; a.pnp_stride = e->post.pnp_stride;
    a.pnp_armor_size = c.armor_size;
    a.cls = e->cls_dev;
    if (e->refined) {   // the guided instantiation: the two live parameters and the prior's buffer
        a.refine = e->refine_dev;
        a.kpts = e->refine_kpts + (size_t)first * c.max_det * 8;
    }
    if (e->pose_alt) {   // the kAlt instantiations: the records beside the step's device records
        a.alts = e->alts.dev_at(first);
        a.prior = e->prior_dev; a.up = e->up_dev;
    }
    return a;
}

static BayerArgs bayer_args(const irmv_engine *e, int first)   // a Bayer engine's demosaic of its raw slots from `first` on
{
    BayerArgs a = e->bayer;
    a.raw = e->raw_dev + (size_t)first * e->src_bytes; a.dst = (e->window ? e->full_dev : e->src_dev) + (size_t)first * e->full_bytes;
    return a;
}

static void launch_bayer(const irmv_engine *e, int first, int count, hipStream_t s)
{
    if (e->bayer_table) launch_demosaic_table(bayer_args(e, first), e->isp_table_dev, e->bayer_mhc, count, s);
    else launch_demosaic(bayer_args(e, first), count, s);
}

PostArgs irmv::post_args(const irmv_engine *e, const View &v, const Step &s)
{
    const int first = s.first;
    PostArgs p = e->post;
    p.scale_x = v.scale_x; p.scale_y = v.scale_y; p.off_x = v.off_x; p.off_y = v.off_y;
    p.head_all = e->head_all;
    p.slots_total = e->cfg.num_slots;
    p.first = first;
    p.boxes = e->boxes + (size_t)first * e->A * 4;
    p.keys = e->keys + (size_t)first * e->A * e->nc;
    p.key_cap = e->A * e->nc;
    p.dets = e->dets.step_at(e, s);
    p.fout = e->fout.step_at(e, s);
    if (p.dbg) p.dbg += (size_t)first * 16;
    p.counts = e->sw.split_scan ? e->cand_counts + first : nullptr;
    p.cand_bits = e->sparse_head ? e->cand_bits + (size_t)first * e->cand_words : nullptr;
    p.cand_words = e->cand_words;
    if (e->pose_alt) {   // nms_pnp_kernel<true>: the alt records go where the DevDet records go
        p.alts = e->alts.step_at(e, s);
        p.prior = e->prior_dev; p.up = e->up_dev;
    }
    return p;
}

// The crop of the step's slots: out of their device frames, or (crop_pinned) out of the pinned slots themselves.
// A tiled step: every slot's window is cut out of tile_frame's device frame.
static CropArgs crop_args(const irmv_engine *e, const Step &s)
{
    CropArgs a{};
    a.src = s.crop_pinned ? e->src_host_dev : e->full_dev; a.src_slot_bytes = e->full_bytes;
    a.dst = e->src_dev; a.dst_slot_bytes = e->frame_bytes;
    a.win = e->win_dev; a.first = s.first;
    a.full_w = e->full_w; a.full_h = e->full_h; a.win_w = e->cfg.src_width; a.win_h = e->cfg.src_height;
    a.src_slot = s.tile_frame;
    return a;
}

static void launch_crop(const irmv_engine *e, const Step &s, hipStream_t st) { launch_window_crop(crop_args(e, s), s.count, st); }

// Frame metering of slots from `first` on in view v: the options at `params`, frame b's record to out[b].
MeterArgs irmv::meter_args(const irmv_engine *e, const View &v, int first, const MeterParams *params, MeterStats *out)
{
    MeterArgs a{};
    a.frames = v.frames; a.frame_bytes = v.frame_bytes;
    a.raw = e->raw_dev; a.raw_bytes = e->src_bytes;
    a.params = params;
    a.win = v.crop ? e->win_dev : nullptr;
    a.slab = e->meter_slab;
    a.out = out;
    a.first = first;
    a.vw = v.src_w; a.vh = v.src_h; a.raw_w = e->full_w; a.raw_h = e->full_h;
    a.rotate180 = e->cfg.rotate180 ? 1 : 0;
    a.ry = e->bayer.ry; a.rx = e->bayer.rx;
    return a;
}

// A step's metering: the records go where its DevDet records go (post_args).  A tiled step does not meter.
static void launch_meter(const irmv_engine *e, const View &v, const Step &s, hipStream_t st)
{
    if (s.tiled()) return;
    launch_frame_meter(meter_args(e, v, s.first, e->meter_params_dev, e->meter.step_at(e, s)), s.count, e->sw.meter_merge, st);
}

static PreArgs pre_args(const irmv_engine *e, const View &v, const Op &op, int first)
{
    PreArgs a;
    a.src = v.frames + (size_t)first * v.frame_bytes;
    a.dst = static_cast<half_t *>(e->tensors[op.out_t].slot(first));
    a.tx = v.tap_x; a.ty = v.tap_y;
    a.sw = v.src_w; a.sh = v.src_h; a.net_w = e->cfg.net_size; a.net_h = e->cfg.net_height; a.swap_rb = e->cfg.swap_rb;
    a.src_slot_bytes = v.frame_bytes;
    return a;
}

static FrontArgs front_args(const irmv_engine *e, const View &v, const Op &op, int first)
{
    FrontArgs a;
    a.src = v.frames + (size_t)first * v.frame_bytes;
    a.src_slot_bytes = v.frame_bytes;
    a.tx = v.tap_x; a.ty = v.tap_y;
    a.vx0 = v.front.box[0]; a.vx1 = v.front.box[1]; a.vy0 = v.front.box[2]; a.vy1 = v.front.box[3];
    a.sw = v.src_w; a.sh = v.src_h; a.net_w = e->cfg.net_size; a.net_h = e->cfg.net_height; a.swap_rb = e->cfg.swap_rb;
    a.fastx = v.front.fastx; a.fx_i0 = v.front.fx_i0; a.fx_step = v.front.fx_step;
    a.w0 = e->conv0_w; a.b0 = e->conv0_b;
    a.w1 = op.w_packed; a.b1 = op.bias;
    const Tensor &ot = e->tensors[op.out_t];
    a.out = static_cast<half_t *>(ot.slot(first));
    a.out_ld = ot.C;
    a.tiles_x = v.front.tiles_x; a.tiles_y = v.front.tiles_y; a.tile_y = v.front.tile_y; a.stage_bytes = v.front.stage_bytes;
    return a;
}

static C2fArgs c2f2_args(const irmv_engine *e, const Op &op, int first)
{
    C2fArgs a;
    const Tensor &xt = e->tensors[op.s0.t], &ot = e->tensors[op.out_t];
    a.x = static_cast<const half_t *>(xt.slot(first)); a.x_ld = xt.C;
    a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
    a.H = xt.H; a.W = xt.W;
    a.tiles_x = (xt.W + kC2fTile - 1) / kC2fTile; a.tiles_y = (xt.H + kC2fTile - 1) / kC2fTile;
    const Op &c1 = e->ops[op.sub[0]], &m1 = e->ops[op.sub[1]], &m2 = e->ops[op.sub[2]], &c2 = e->ops[op.sub[3]];
    a.w_cv1 = c1.w_packed; a.w_m1 = m1.w_packed; a.w_m2 = m2.w_packed; a.w_cv2 = c2.w_packed;
    a.b_cv1 = c1.bias; a.b_m1 = m1.bias; a.b_m2 = m2.bias; a.b_cv2 = c2.bias;
    return a;
}

// one fused C2f block (OP_C2F32).  (A 16 x 16 tile on an 8-wave workgroup -- a third less halo work, one workgroup per CU --
// was built and measured in round 3: 5 - 30 % slower than the 8 x 16 tile in an eager replay, a tie in the benchmarked one;
// dropped.)
static C2f32Args c2f32_args(const irmv_engine *e, const Op &op, int first, int count)
{
    C2f32Args a{};
    const Tensor &ct = e->tensors[op.res_t];
    const Tensor &ot = e->tensors[op.out_t];
    if (op.sub[0] >= 0) {
        ConvArgs ca;
        fill_conv_args(e, e->ops[op.sub[0]], first, count, ca, false);
        a.s0 = ca.s0; a.s1 = ca.s1; a.cin1 = ca.Cin;
        a.w_cv1 = e->ops[op.sub[0]].w_packed; a.b_cv1 = e->ops[op.sub[0]].bias;
    } else {
        a.cin1 = 32;
    }
    a.cat = static_cast<half_t *>(ct.slot(first)); a.cat_ld = ct.C; a.prev_coff = 64;
    a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
    a.H = op.Hin; a.W = op.Win;
    a.tiles_x = (op.Win + kC2f32TileW - 1) / kC2f32TileW; a.tiles_y = (op.Hin + kC2f32TileH - 1) / kC2f32TileH;
    a.w_m1 = e->ops[op.sub[1]].w_packed; a.b_m1 = e->ops[op.sub[1]].bias;
    a.w_m2 = e->ops[op.sub[2]].w_packed; a.b_m2 = e->ops[op.sub[2]].bias;
    if (op.sub[3] >= 0) { a.w_cv2 = e->ops[op.sub[3]].w_packed; a.b_cv2 = e->ops[op.sub[3]].bias; }
    return a;
}

static BneckArgs bneck_args(const irmv_engine *e, const Op &op, int first)
{
    const Op &m1 = e->ops[op.sub[0]], &m2 = e->ops[op.sub[1]];
    const Tensor &ct = e->tensors[op.res_t];
    BneckArgs a{};
    a.yin = static_cast<const half_t *>(ct.slot(first)) + m1.s0.coff; a.yin_ld = ct.C;
    a.ynext = static_cast<half_t *>(ct.slot(first)) + m2.out_coff; a.ynext_ld = ct.C;
    a.cat = static_cast<const half_t *>(ct.slot(first)); a.cat_ld = ct.C;
    a.H = op.Hin; a.W = op.Win;
    a.tiles_x = (op.Win + kBneckTile - 1) / kBneckTile; a.tiles_y = (op.Hin + kBneckTile - 1) / kBneckTile;
    a.w_m1 = m1.w_lds[0]; a.b_m1 = m1.bias; a.w_m2 = m2.w_lds[0]; a.b_m2 = m2.bias;
    if (op.sub[2] >= 0) {
        const Op &c2 = e->ops[op.sub[2]];
        const Tensor &ot = e->tensors[c2.out_t];
        a.out = static_cast<half_t *>(ot.slot(first)) + c2.out_coff; a.out_ld = ot.C;
        a.w_cv2 = c2.w_packed; a.b_cv2 = c2.bias;
    }
    return a;
}

static Kpt3Args kpt3_args(const irmv_engine *e, const Op &op, const Launch &l, int first, const PostArgs &pa)
{
    const Op &o0 = e->ops[op.sub[0]], &o1 = e->ops[op.sub[1]], &o2 = e->ops[op.sub[2]];
    const Tensor &xt = e->tensors[o0.s0.t], &ht = e->tensors[o2.out_t];
    Kpt3Args a{};
    a.x = static_cast<const half_t *>(xt.slot(first)) + o0.s0.coff; a.x_ld = xt.C;
    a.H = op.Hin; a.W = op.Win;
    a.tiles_x = (op.Win + kKpt3Tile - 1) / kKpt3Tile; a.tiles_y = (op.Hin + kKpt3Tile - 1) / kKpt3Tile;
    a.w1 = o0.w_lds[0]; a.b1 = o0.bias;
    a.w2 = o1.w_packed; a.b2 = o1.bias;
    a.w3 = o2.w_k16; a.b3 = o2.bias;
    a.out = static_cast<float *>(ht.slot(first)) + o2.out_coff; a.out_ld = ht.C;
    if (l.sparse) { a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words; a.abase = e->lvl_base[op.level]; a.tile_gate = l.gate; }
    return a;
}

// the candidate lists of slots [first, first + count): every level that has an OP_BOXG op
static CandListArgs cand_list_args(const irmv_engine *e, int first, const PostArgs &pa)
{
    CandListArgs a{};
    a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words;
    const size_t S = (size_t)e->cfg.num_slots;
    for (int l = 0; l < 3; l++) { a.abase[l] = e->lvl_base[l]; a.hw[l] = e->lvl_hw[l]; }
    for (const Op &op : e->ops)
        if (op.kind == OP_BOXG) {
            const int l = op.level;
            a.list[l] = e->boxg_list + (size_t)e->lvl_base[l] * S + (size_t)first * e->lvl_hw[l];
            a.count[l] = e->boxg_count + (size_t)l * S + first;
        }
    return a;
}

static BoxGatherArgs boxg_args(const irmv_engine *e, const Op &op, const Launch &l, int first, const PostArgs &pa)
{
    const Op &o0 = e->ops[op.sub[0]], &o1 = e->ops[op.sub[1]], &o2 = e->ops[op.sub[2]];
    const Tensor &xt = e->tensors[o0.s0.t], &ht = e->tensors[o2.out_t];
    const CandListArgs c = cand_list_args(e, first, pa);
    BoxGatherArgs a{};
    a.x = static_cast<const half_t *>(xt.slot(first)) + o0.s0.coff; a.x_ld = xt.C;
    a.H = op.Hin; a.W = op.Win;
    a.w0 = o0.w_lds[2]; a.b0 = o0.bias;
    a.w1 = o1.w_lds[2]; a.b1 = o1.bias;
    a.w2 = o2.w_packed; a.b2 = o2.bias;
    a.out = static_cast<float *>(ht.slot(first)) + o2.out_coff; a.out_ld = ht.C;
    a.list = c.list[op.level]; a.count = c.count[op.level];
    if (l.kpt >= 0) {   // the keypoint branch rides along: kpt3_args' operands
        const Op &k = e->ops[l.kpt];
        const Op &k0 = e->ops[k.sub[0]], &k1 = e->ops[k.sub[1]], &k2 = e->ops[k.sub[2]];
        const Tensor &kt = e->tensors[k2.out_t];
        a.kw0 = k0.w_lds[0]; a.kb0 = k0.bias;
        a.kw1 = k1.w_packed; a.kb1 = k1.bias;
        a.kw2 = k2.w_k16; a.kb2 = k2.bias;
        a.kout = static_cast<float *>(kt.slot(first)) + k2.out_coff; a.kout_ld = kt.C;
    }
    return a;
}

static DwArgs dw_args(const irmv_engine *e, const Op &op, int first)
{
    DwArgs a;
    const Tensor &xt = e->tensors[op.s0.t], &ot = e->tensors[op.out_t];
    a.x = static_cast<const half_t *>(xt.slot(first)) + op.s0.coff; a.x_ld = xt.C;
    a.y = static_cast<half_t *>(ot.slot(first)) + op.out_coff; a.y_ld = ot.C;
    a.w = op.w_packed; a.b = op.bias;
    a.Hin = op.Hin; a.Win = op.Win; a.Hout = op.Hout; a.Wout = op.Wout; a.C = op.cout; a.stride = op.cfg.stride;
    return a;
}

static ShufArgs shuf_args(const irmv_engine *e, const Op &op, int first, int count)
{
    ShufArgs a;
    const Tensor &at = e->tensors[op.s0.t], &bt = e->tensors[op.s1.t], &ot = e->tensors[op.out_t];
    a.a = static_cast<const half_t *>(at.slot(first)) + op.s0.coff; a.a_ld = at.C;
    a.b = static_cast<const half_t *>(bt.slot(first)) + op.s1.coff; a.b_ld = bt.C;
    a.out = static_cast<half_t *>(ot.slot(first)); a.out_ld = ot.C;
    a.bc = op.s0.C;
    a.pixels = (size_t)count * op.Hin * op.Win;
    return a;
}

static Conv0Args conv0_args(const irmv_engine *e, const Op &op, int first, int count)
{
    Conv0Args a;
    a.x = static_cast<const half_t *>(e->tensors[op.s0.t].slot(first));
    a.y = static_cast<half_t *>(e->tensors[op.out_t].slot(first));
    a.w = e->conv0_w; a.b = e->conv0_b; a.net_w = e->cfg.net_size; a.net_h = e->cfg.net_height; a.batch = count;
    return a;
}

// ---- grouped Detect-branch launches (single-frame engines) ---------------------------

static void scan_args_for(const irmv_engine *e, const Op &op, const PostArgs &pa, ConvArgs &a)
{
    a.scan_keys = pa.keys; a.scan_counts = pa.counts; a.scan_cls = pa.cls; a.scan_nc = pa.nc;
    a.scan_key_cap = pa.key_cap;
    a.scan_abase = e->lvl_base[op.level];
    a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words;   // (sparse head: the class channels stay on chip)
}

// one launch for all members of group g on slot `first`; member k appends candidates to pa's key lists if bit k of `scan` is set
bool irmv::launch_head_group(const irmv_engine *e, const irmv_engine::HeadGroup &g, int first, const PostArgs *pa, unsigned scan, hipStream_t s)
{
    ConvArgs a[kMultiMax];
    ConvWeights w[kMultiMax];
    const int n = (int)g.members.size();
    for (int k = 0; k < n; k++) {
        const Op &op = e->ops[g.members[k]];
        fill_conv_args(e, op, first, 1, a[k], true);
        if (scan >> k & 1u) scan_args_for(e, op, *pa, a[k]);
        w[k] = conv_weights(op);
    }
    return g.family == 0 ? launch_conv_lds_multi(g.nt, a, w, n, 1, s) : launch_conv_direct_multi(g.cfg, a, n, s);
}

// ---- step execution ------------------------------------------------------------
// The one place an op reaches the GPU: the kernel of l.op's kind on the slots of step t, stream s, as launch l of a plan of
// view v says (irmv_engine_run_op: a plain Launch of the op).  scan: the members of l that append scan candidates to pa's key
// lists (bit k: member k of a group, bit 0: a lone conv).  A tiled step differs in OP_DEMOSAIC and OP_CROP only (Step).
int irmv::launch_op(irmv_engine *e, const View &v, const Launch &l, const Step &t, const PostArgs &pa, unsigned scan, hipStream_t s)
{
    const Op &op = e->ops[l.op];
    const int first = t.first, count = t.count;
    switch (op.kind) {
    case OP_DEMOSAIC: launch_bayer(e, t.bayer_first(), t.bayer_count(), s); break;
    case OP_CROP: launch_crop(e, t, s); break;
    case OP_METER: launch_meter(e, v, t, s); break;
    case OP_YAW: launch_yaw(e, t, pa, s); break;
    case OP_POSECOV: launch_posecov(e, t, pa, s); break;
    case OP_PATCH: launch_patch(e, v, t, pa, s); break;
    case OP_NUMBER: launch_number(e, t, pa, s); break;
    case OP_PRE: launch_preprocess(pre_args(e, v, op, first), count, s); break;
    case OP_FRONT: if (!launch_front(front_args(e, v, op, first), count, s)) return fail(IRMV_ERR_HIP, "fused front kernel: LDS request refused"); break;
    case OP_C2F2: launch_c2f2(c2f2_args(e, op, first), count, s); break;
    case OP_C2F32: if (!launch_c2f32(op.mode, op.shortcut, c2f32_args(e, op, first, count), count, s)) return fail(IRMV_ERR_ARG, "no fused C2f kernel for " + op.layer); break;
    case OP_BNECK:   // (cv2's k-steps where the launch carries it)
        if (!launch_bneck64(op.mode, op.sub[2] >= 0 ? e->ops[op.sub[2]].ksteps : 6, op.shortcut, bneck_args(e, op, first), count, s)) return fail(IRMV_ERR_ARG, "no fused bottleneck kernel for " + op.layer);
        break;
    case OP_KPT3: if (!launch_kpt3(kpt3_args(e, op, l, first, pa), op.cin, count, s)) return fail(IRMV_ERR_ARG, "no fused keypoint-branch kernel for " + op.layer); break;
    case OP_BOXG:
        if (!pa.cand_bits) return fail(IRMV_ERR_ARG, "a box gather launch needs the sparse head's bitmap: " + op.layer);
        if (l.cand_list) launch_cand_list(cand_list_args(e, first, pa), count, s);
        if (!launch_box_gather(boxg_args(e, op, l, first, pa), op.cin, count, l.grid > 0 ? l.grid : (e->sw.gather_grid > 0 ? e->sw.gather_grid : e->num_cus), s)) return fail(IRMV_ERR_ARG, "no box gather kernel for " + op.layer);
        break;
    case OP_DW: launch_dwconv3x3(dw_args(e, op, first), count, s); break;
    case OP_SHUF: launch_shuffle_cat(shuf_args(e, op, first, count), s); break;
    case OP_CONV0: launch_conv0(conv0_args(e, op, first, count), s); break;
    case OP_POOL: { const Tensor &t = e->tensors[op.out_t]; launch_sppf_pool(static_cast<half_t *>(t.slot(first)), count, t.H, t.W, t.C / 4, s); break; }
    case OP_CONV: {
        if (l.group >= 0) {
            if (!launch_head_group(e, e->head_groups[l.group], first, &pa, scan, s)) return fail(IRMV_ERR_ARG, "grouped launch refused: " + l.name);
            break;
        }
        ConvArgs a;
        fill_conv_args(e, op, first, count, a, l.fused);
        if (scan) scan_args_for(e, op, pa, a);
        if (l.sparse || l.gate) { a.cand_bits = pa.cand_bits; a.cand_words = pa.cand_words; a.scan_abase = e->lvl_base[op.level]; a.tile_gate = l.gate; }
        if (!run_conv(op, l.cfg_one ? op.cfg_one : op.cfg, a, count, s)) return fail(IRMV_ERR_ARG, std::string("no conv kernel for ") + op.kname + " (" + op.layer + ")");
        break;
    }
    case OP_SCAN: launch_scan_decode(pa, count, s); break;
    case OP_NMS: { PostArgs pn = pa; pn.keys_only = l.keys_only ? 1 : 0; launch_nms_pnp(pn, count, s); break; }
    case OP_LIGHT: launch_light_extract(light_args(e, v, first), e->cfg.max_det, count, s); break;
    }
    HIP_TRY(hipGetLastError());
    return IRMV_OK;
}

// Enqueue step t on stream s: the launches of its kind's plan in its slots' view (the caller has made sure they share one),
// in order; behind them, in a tiled step, the merge of the slots' lists (k_tiles.hip).
// ev != nullptr (irmv_engine_profile's events): launch i of the plan is repeated `reps` times (once if it is `once`) between
// (*ev)[2 i] and (*ev)[2 i + 1].
int irmv::enqueue_step(irmv_engine *e, const Step &t, hipStream_t s, int reps, const std::vector<hipEvent_t> *ev)
{
    const View &v = view_of(e, t.first);
    const std::vector<Launch> &plan = v.plans[t.kind];
    const PostArgs pa = post_args(e, v, t);
    PostArgs mute = pa;   // (the table's twin with thresholds no logit passes: no key, no bit)
    mute.cls = e->cls_dev + 1;
    for (size_t i = 0; i < plan.size(); i++) {
        const Launch &l = plan[i];
        if (ev) HIP_TRY(hipEventRecord((*ev)[2 * i], s));
        const int n = l.once ? 1 : reps;
        for (int rep = 0; rep < n; rep++) {
            // a profiled launch is repeated: only its last repetition appends candidates.  With the sparse head the other
            // repetitions still run the step's kernel -- no class store --, behind the mute threshold.
            const bool last = rep == n - 1, muted = !last && l.scan && e->sparse_head;
            TRY(launch_op(e, v, l, t, muted ? mute : pa, last || muted ? l.scan : 0u, s));
        }
        if (ev) HIP_TRY(hipEventRecord((*ev)[2 * i + 1], s));
    }
    if (t.tiled()) {
        launch_tile_merge(tile_args(e, t.first, t.count), s);
        HIP_TRY(hipGetLastError());
    }
    return IRMV_OK;
}

// The corners and views of slots [first, first + count) as of this submit (or merge): what their results are shifted by from
// here on -- the windows' corners as they are now, or, in the frame view, nothing.
void irmv::note_submit_windows(irmv_engine *e, int first, int count)
{
    if (!e->window) return;
    std::copy(e->win_org.begin() + first, e->win_org.begin() + first + count, e->sub_org.begin() + first);
    std::copy(e->slot_view.begin() + first, e->slot_view.begin() + first + count, e->sub_view.begin() + first);
}

// Slots [first, first + count) have just been stepped: their heads hold the rows, and their gated tensors the tiles, of that
// step's candidates only (sparse head / branch).
void irmv::mark_stepped(irmv_engine *e, int first, int count)
{
    if (e->sparse_head) std::fill(e->head_stale.begin() + first, e->head_stale.begin() + first + count, 1);
    if (e->sparse_branch) std::fill(e->branch_stale.begin() + first, e->branch_stale.begin() + first + count, 1);
    note_submit_windows(e, first, count);
}

// Frame upload and result download: pinned memory both ways, on the streams submit_group() picks.
// One or two frames travel from the pinned slots as a KERNEL (k_pre.hip upload_frame_kernel), larger groups on the copy engine.
static bool upload_as_kernel(const irmv_engine *e, int first, int count)
{
    return count <= 2 && e->sw.upload_kernel_blocks > 0 && e->src_host_dev && upload_aligned(e->src_bytes, first, count);
}

// THE decision of how the pinned frames of slots [first, first + count) reach the device; whoever uploads asks once and hands
// the answer on (enqueue_upload, get_graph, Step::crop_pinned).
// copy_engine: the upload rides the side stream, or stands outside a step (load_frame): never a kernel, never nothing.
// captured: the upload becomes a graph node, whose copy parameters are baked: never bands.
// tile_frame >= 0 (a tiled step): that slot's frame, whole -- never bands, never the crop out of the pinned slot.
// Otherwise, in order:
//   - an HWC window engine's step of one or two slots in the window view uploads nothing: its crop reads the window out of the
//     pinned slots, so only the window crosses PCIe (IRMV_WINDOW_UPLOAD=0: off);
//   - the upload kernel.  (A Bayer engine's single-frame upload stays a kernel of its own in front of the demosaic: the demosaic
//     reading the pinned slot itself was built and measured slower)
//   - bands: an HWC window engine moves, for groups of up to 8 slots in the window view, only the band of full-width rows each
//     slot's window covers;
//   - one copy of the whole frames (every slot in the frame view, every Bayer engine).
constexpr int kBandUploadMaxSlots = 8;
Upload irmv::choose_upload(const irmv_engine *e, int first, int count, int tile_frame, bool copy_engine, bool captured)
{
    if (tile_frame >= 0) return {!copy_engine && upload_as_kernel(e, tile_frame, 1) ? UP_KERNEL : UP_COPY, tile_frame, 1};
    const bool hwc_window = view_of(e, first).crop && !e->raw_dev;
    if (!copy_engine) {
        if (hwc_window && e->sw.window_upload && count <= 2 && e->sw.upload_kernel_blocks > 0 && e->src_host_dev) return {UP_PINNED_CROP, first, count};
        if (upload_as_kernel(e, first, count)) return {UP_KERNEL, first, count};
    }
    return {hwc_window && count <= kBandUploadMaxSlots && !captured ? UP_BANDS : UP_COPY, first, count};
}

int irmv::enqueue_upload(irmv_engine *e, const Upload &u, hipStream_t st)
{
    const size_t off = (size_t)u.first * e->src_bytes, bytes = e->src_bytes * u.count;
    switch (u.form) {
    case UP_NONE: case UP_PINNED_CROP: break;
    case UP_KERNEL: launch_upload_frames(e->src_host_dev + off, upload_dev(e) + off, bytes, e->sw.upload_kernel_blocks, st); break;
    case UP_COPY: HIP_TRY(hipMemcpyAsync(upload_dev(e) + off, e->src_host + off, bytes, hipMemcpyHostToDevice, st)); break;
    case UP_BANDS: {   // one 1-D copy per slot, to the same offset of its device frame
        const size_t pitch = (size_t)e->full_w * 3, len = (size_t)e->cfg.src_height * pitch;
        for (int s = u.first; s < u.first + u.count; s++) {
            const int by0 = e->cfg.rotate180 ? e->full_h - e->win_org[s].y - e->cfg.src_height : e->win_org[s].y;
            const size_t boff = (size_t)s * e->src_bytes + (size_t)by0 * pitch;
            HIP_TRY(hipMemcpyAsync(e->full_dev + boff, e->src_host + boff, len, hipMemcpyHostToDevice, st));
        }
        break;
    }
    }
    return IRMV_OK;
}

// ---- record channels (Records<T>, engine_internal.hpp) ---------------------------------------
// Pin: in this order the device range is zeroed, the pinned twin made, its device view fetched, the twin zeroed and logged.
template <typename T> int Records<T>::pin(const irmv_engine *e, int slots, int n_per_slot, const char *what)
{
    per_slot = n_per_slot;
    const size_t bytes = (size_t)slots * per_slot * sizeof(T);
    HIP_TRY(hipMemset(dev, 0, bytes));
    HIP_TRY(hipHostMalloc((void **)&host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void **)&host_dev, host, 0));
    memset(host, 0, bytes);
    log_range(e, what, host, bytes);
    return IRMV_OK;
}

// THE decision of where a step's records go: into pinned host memory where the engine's results are zero-copy, unless a kernel
// behind the writer reads them on the device (Step::dev_records) -- then, and on every other engine, into the device records,
// and copy_out_dev brings them to the host.
template <typename T> T *Records<T>::step_at(const irmv_engine *e, const Step &s) const
{
    return (e->zero_copy_results && !s.dev_records() ? host_dev : dev) + (size_t)s.first * per_slot;
}

template <typename T> int Records<T>::copy(int first, int count, hipMemcpyKind dir, hipStream_t st) const
{
    const size_t at = (size_t)first * per_slot, bytes = (size_t)count * per_slot * sizeof(T);
    if (dir == hipMemcpyDeviceToHost) HIP_TRY(hipMemcpyAsync(host + at, dev + at, bytes, dir, st));
    else HIP_TRY(hipMemcpyAsync(dev + at, host + at, bytes, dir, st));
    return IRMV_OK;
}

template <typename T> int Records<T>::zero(int slots) const
{
    const size_t bytes = (size_t)slots * per_slot * sizeof(T);
    HIP_TRY(hipMemset(dev, 0, bytes));
    memset(host, 0, bytes);
    return IRMV_OK;
}

template <typename T> int Records<T>::deliver(const irmv_engine *e, int slot, void *out, int cap, int *n) const
{
    const int k = std::max(0, std::min(std::min(e->fout.host_at(slot)->num_dets, e->cfg.max_det), cap));
    if (k) memcpy(out, host_at(slot), (size_t)k * sizeof(T));
    *n = k;
    return IRMV_OK;
}

template <typename T> void Records<T>::free_host()
{
    if (host) (void)hipHostFree(host);
    host = host_dev = nullptr;
}

template struct Records<MeterStats>;
template struct Records<DevDet>;
template struct Records<DevFrameOut>;
template struct Records<DevAlt>;
template struct Records<DevYaw>;
template struct Records<DevPoseCov>;
template struct Records<DevPatch>;
template struct Records<DevNumber>;
template struct Records<DevDetTrack>;
template struct Records<DevTrackSnap>;

// the device records of slots [first, first + count) -> their pinned twins (every step of an engine without zero-copy results;
// tiled steps of any engine -- which do not meter: stats = false)
static int copy_out_dev(irmv_engine *e, int first, int count, hipStream_t st, bool stats)
{
    const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
    if (stats && e->meter_op >= 0) TRY(e->meter.copy(first, count, d2h, st));
    TRY(e->dets.copy(first, count, d2h, st));
    TRY(e->fout.copy(first, count, d2h, st));
    if (e->pose_alt) TRY(e->alts.copy(first, count, d2h, st));
    if (e->yaw_op >= 0) TRY(e->yaw.copy(first, count, d2h, st));
    if (e->posecov_op >= 0 && e->posecov_opts.enable) TRY(e->posecov.copy(first, count, d2h, st));   // (disabled: as the patches)
    // (disabled: the kernel returns at once and set_patches has zeroed both copies -- max_det records of 592 bytes stay where they are)
    if (e->patch_op >= 0 && e->patch_opts.enable) TRY(e->patch.copy(first, count, d2h, st));
    if (e->number_op >= 0 && e->number_opts.enable) TRY(e->number.copy(first, count, d2h, st));   // (disabled: as the patches)
    // (disabled: nothing is launched and set_tracking has zeroed both copies)
    if (e->track_made && e->track_opts.enable) {
        TRY(e->dettrack.copy(first, count, d2h, st));
        TRY(e->tracks.copy(first, count, d2h, st));
    }
    return IRMV_OK;
}

int irmv::copy_out(irmv_engine *e, int first, int count, hipStream_t st)
{
    if (e->zero_copy_results) return IRMV_OK;   // the kernel has already written the pinned records
    return copy_out_dev(e, first, count, st ? st : e->stream, true);
}

int irmv::check_range(const irmv_engine *e, int first, int count)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (first < 0 || count < 1 || first + count > e->cfg.num_slots) return fail(IRMV_ERR_ARG, "slot range out of bounds");
    return IRMV_OK;
}

// The captured graph of step s in its slots' present view.  upload (choose_upload's answer with `captured`; UP_NONE: none): the
// frames' upload as the graph's first node (synchronous single-stream submits).
int irmv::get_graph(irmv_engine *e, const Step &s, const Upload &upload, hipGraphExec_t *out)
{
    const GraphKey key{s, upload.form != UP_NONE, e->slot_view[s.first]};
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) { *out = it->second; return IRMV_OK; }
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_upload(e, upload, e->stream);
    if (!rc) rc = enqueue_step(e, s, e->stream);
    hipError_t ce = hipStreamEndCapture(e->stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (ce != hipSuccess) return fail(IRMV_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    hipGraphExec_t ge = nullptr;
    HIP_TRY(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    e->graphs[key] = ge;
    *out = ge;
    return IRMV_OK;
}

static int group_of(irmv_engine *e, int first, int count, SlotGroup **out)
{
    const auto key = std::make_pair(first, count);
    auto it = e->groups.find(key);
    if (it == e->groups.end()) {
        SlotGroup g;
        g.first = first; g.count = count;
        HIP_TRY(hipEventCreateWithFlags(&g.h2d, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.out, hipEventDisableTiming));
        it = e->groups.emplace(key, g).first;
    }
    *out = &it->second;   // std::map nodes never move
    return IRMV_OK;
}

// One slot group: [upload] -> ONE hipGraph -> download of the results, in order on compute stream `st`.
//
// IRMV_SUBMIT_ASYNC_UPLOAD moves the upload to the engine's upload stream (the dGPU form of the
// reference's TripleBuffer, include/irmv_detection/triple_buffer.hpp:24-40, whose slots ARE the engines' input memory):
//
//   upload stream    [wait: this group's previous step is done with its device frames]  H2D frames  -> ev h2d
//   compute stream   [wait: ev h2d]  hipGraph, D2H results                                           -> ev out
//
// so group B's frames cross PCIe while group A's kernels run.  The price is one cross-stream event hop per group
// (measured on this stack: scripts/probes/stream_probe.cpp), which is why a lone synchronous detect() -- nothing to
// overlap with -- keeps everything on one stream, and why the (tiny) download never leaves the compute stream.
//
// tile_frame >= 0: a tiled step (irmv_engine_submit_tiles) of the group on that slot's frame.  The same path with other data:
// tile_frame counts as touched, so a later upload into it waits for this step and this step for whatever touched it last; the
// caller passes compute stream 0; the step is never eager; its records are device records, copied out on every engine; and the
// merged list's record (TileOut) follows them in front of event `out`.
int irmv::submit_group(irmv_engine *e, int f, int c, uint32_t flags, hipStream_t st, int tile_frame)
{
    const bool tiled = tile_frame >= 0, h2d = (flags & IRMV_SUBMIT_H2D) != 0;
    const bool async_up = h2d && (flags & IRMV_SUBMIT_ASYNC_UPLOAD) && !e->sw.inline_copies;
    // An upload that rides the compute stream anyway (the synchronous detect()) is captured INTO the step's graph: one
    // submission instead of two, and the copy -> first kernel hand-over is the graph's own (IRMV_GRAPH_UPLOAD=0: a separate
    // hipMemcpyAsync in front of the graph, as before; same bits)
    // A synchronous single-frame step (the reference's detect(), src/yolo_engine.cpp:153-177) has two launch forms with the same
    // kernels and the same bits: ONE hipGraph replay, or its 41 launches issued one by one behind the upload (round 5: a graph
    // replay spends ~10 us of host work before its first packet reaches the GPU, a direct launch ~4; with the 70 us upload in
    // front the host stays far ahead of the GPU: 0.339 -> 0.331 ms per 1280 x 1024 frame).  Every other step is a graph replay.
    const bool eager = !tiled && e->sync_launch == 1 && c == 1 && h2d && !async_up;
    // The upload's form, asked once: every use below is this answer.  (`captured` is graph_up wherever the answer depends on it.)
    const Upload upload = h2d ? choose_upload(e, f, c, tile_frame, async_up, !async_up && e->sw.graph_upload && !eager) : Upload{};
    const bool pinned = upload.form == UP_PINNED_CROP;   // (no upload at all: nothing to keep out of the graph)
    const bool graph_up = h2d && !async_up && (e->sw.graph_upload || pinned) && !eager;
    const Step step{c == 1 ? STEP_ONE : STEP_BATCH, f, c, tile_frame, pinned};
    hipGraphExec_t ge = nullptr;
    if (!eager) TRY(get_graph(e, step, graph_up ? upload : Upload{}, &ge));
    SlotGroup *g;
    TRY(group_of(e, f, c, &g));
    hipStream_t up = async_up ? e->h2d_stream : st;
    // slots last used through a different grouping (a tiled step: the frame's owner too): order behind that group's completion
    SlotGroup *seen[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < c + (tiled ? 1 : 0); i++) {
        const int s = i < c ? f + i : tile_frame;
        SlotGroup *o = e->slot_owner[s];
        e->slot_owner[s] = g;
        if (!o || o == g || !o->in_flight || o == seen[0] || o == seen[1] || o == seen[2] || o == seen[3]) continue;
        seen[3] = seen[2]; seen[2] = seen[1]; seen[1] = seen[0]; seen[0] = o;
        if (o->compute != st) HIP_TRY(hipStreamWaitEvent(st, o->out, 0));
        if (up != st) HIP_TRY(hipStreamWaitEvent(up, o->out, 0));
    }
    if (g->in_flight && g->compute != st) HIP_TRY(hipStreamWaitEvent(st, g->out, 0));   // the group moved to another compute stream
    if (async_up) {
        if (g->in_flight) HIP_TRY(hipStreamWaitEvent(up, g->out, 0));   // previous step has consumed the device frames
        TRY(enqueue_upload(e, upload, up));
        HIP_TRY(hipEventRecord(g->h2d, up));
        HIP_TRY(hipStreamWaitEvent(st, g->h2d, 0));
    } else if (!graph_up) {
        // (an eager step, or IRMV_GRAPH_UPLOAD=0; a submit without IRMV_SUBMIT_H2D: UP_NONE)
        TRY(enqueue_upload(e, upload, st));
    }
    if (eager) TRY(enqueue_step(e, step, st));
    else HIP_TRY(hipGraphLaunch(ge, st));
    mark_stepped(e, f, c);
    // the track table advances behind the step, in submit order (rule 7); a tiled step does not feed it
    if (tiled) TRY(track_skip(e, f, c, st, true));   // (copy_out_dev below carries the zeros)
    else TRY(track_step(e, step, st));
    if (tiled) {
        const irmv_engine::TileMerge &tm = e->tile_merges.at(f);
        TRY(copy_out_dev(e, f, c, st, false));
        HIP_TRY(hipMemcpyAsync(tm.out_host, tm.out_dev, sizeof(TileOut), hipMemcpyDeviceToHost, st));
    } else {
        TRY(copy_out(e, f, c, st));
    }
    HIP_TRY(hipEventRecord(g->out, st));
    g->in_flight = true;
    g->async_up = async_up;
    g->compute = st;
    return IRMV_OK;
}

extern "C" int irmv_engine_submit(irmv_engine *e, int first, int count, uint32_t flags)
{
    TRY(check_range(e, first, count));
    TRY(slots_view(e, first, count));   // (before anything is enqueued)
    HIP_TRY(hipSetDevice(e->cfg.device));
    // A multi-slot step is cut into num_streams independent sub-batches, one captured graph each, on
    // separate streams: while one sub-batch sits in a launch gap or a kernel tail the other keeps the
    // CUs busy (two sub-batches measured +30 % frames/s over one stream at 32 frames).
    int share = count > 1 ? stream_share(e, count) : count;
    // Single-slot steps ride the compute stream of their slot (slot mod num_streams): a single frame fills a fraction of
    // the chip, so the steps of two slots in flight (the TripleBuffer's depth) overlap instead of queueing behind each other.
    int si = count == 1 ? first % e->num_streams : 0;
    // A submit of exactly ONE stream's share of the engine's slots, aligned to it, is that share's sub-batch of a whole-engine
    // step: the same captured graph on the same stream.  A caller that feeds the shares separately decides itself how far
    // apart the streams run (two shares started together execute the same kernel at the same time all the way down).
    const int full_share = stream_share(e, e->cfg.num_slots);
    if (count > 1 && count == full_share && first % full_share == 0 && first / full_share < e->num_streams) { share = count; si = first / full_share; }
    for (int f = first; f < first + count; f += share, si++) {
        const int c = std::min(share, first + count - f);
        hipStream_t st = si == 0 ? e->stream : e->extra_streams[si - 1];
        TRY(submit_group(e, f, c, flags, st));
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_run_post(irmv_engine *e, int first, int count)
{
    TRY(check_range(e, first, count));
    TRY(slots_view(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    for (int s = first; s < first + count; s++) TRY(ensure_dense_head(e, s));   // (scan_decode_kernel reads every anchor's class logits)
    hipGraphExec_t ge;
    TRY(get_graph(e, Step{STEP_POST, first, count}, Upload{}, &ge));
    HIP_TRY(hipGraphLaunch(ge, e->stream));
    TRY(track_skip(e, first, count, e->stream, !e->zero_copy_results));   // (run_post does not feed the tracker; copy_out below copies iff the results are not zero-copy)
    TRY(copy_out(e, first, count));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

extern "C" int irmv_engine_wait(irmv_engine *e)
{
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(e->h2d_stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 1; i < e->num_streams; i++) HIP_TRY(hipStreamSynchronize(e->extra_streams[i - 1]));
    for (auto &kv : e->groups) kv.second.in_flight = false;
    return IRMV_OK;
}

// Block until the last submit of slots [first, first + count) has got as far as `upload` says: their pinned slots have been read
// by its upload, or its results are host-visible.
static int wait_owners(irmv_engine *e, int first, int count, bool upload)
{
    TRY(check_range(e, first, count));
    HIP_TRY(hipSetDevice(e->cfg.device));
    SlotGroup *last = nullptr;
    for (int s = first; s < first + count; s++) {
        SlotGroup *o = e->slot_owner[s];
        if (!o || o == last || !o->in_flight) continue;
        // an upload on the side stream has its own event; an inline upload is ordered in front of the kernels, so the
        // group's completion event covers it
        HIP_TRY(hipEventSynchronize(upload && o->async_up ? o->h2d : o->out));
        // the whole group is done only if this call covers it; otherwise it merely stays marked in flight (harmless)
        if (!upload && o->first >= first && o->first + o->count <= first + count) o->in_flight = false;
        last = o;
    }
    return IRMV_OK;
}

// From then on a producer may overwrite the pinned slots (the moment the TripleBuffer's consumer can give the buffer back),
// while the kernels still run.
extern "C" int irmv_engine_wait_upload(irmv_engine *e, int first, int count) { return wait_owners(e, first, count, true); }

// Other slots may stay in flight (the consumer side of the TripleBuffer: take the newest finished slot while the next one runs).
extern "C" int irmv_engine_wait_slots(irmv_engine *e, int first, int count) { return wait_owners(e, first, count, false); }

// The pose part of a result record: keypoints (shift: a window's, moved by the corner ox, oy), PnP, and the classical
// extraction's fields.
void irmv::det_pose(const DevDet &d, bool shift, float ox, float oy, irmv_det &o)
{
    o.pnp_ok = d.pnp_ok;
    memcpy(o.kpts, d.kpts, 32);
    if (shift)
        for (int j = 0; j < 8; j++) o.kpts[j] += (j & 1) ? oy : ox;
    memcpy(o.rvec, d.rvec, 24);
    memcpy(o.tvec, d.tvec, 24);
    memcpy(o.quat, d.quat, 32);
    o.armor_valid = d.armor_valid;
    o.armor_size = d.armor_size;
    o.n_lights = d.n_lights;
}

// Record i of the slot's pinned result list as the ABI returns it (irmv_engine_results, irmv_engine_tile_results).
void irmv::slot_det(const irmv_engine *e, int slot, int i, irmv_det &o)
{
    const DevDet &d = e->dets.host_at(slot)[i];
    // device records of a step in the window view are window-local: the corner the slot was submitted with brings them to
    // full-frame coordinates (a step in the frame view: nothing to add)
    const bool shift = e->window && e->sub_view[slot] == IRMV_VIEW_WINDOW;
    const float ox = shift ? (float)e->sub_org[slot].x : 0.f, oy = shift ? (float)e->sub_org[slot].y : 0.f;
    memcpy(o.xyxy, d.xyxy, 16);
    o.score = d.score;
    // magic_enum::enum_cast<ArmorClass>(label).value_or(UNKNOWN), src/yolo_engine.cpp:216
    o.class_id = (d.cls >= 0 && d.cls < IRMV_NUM_CLASSES) ? d.cls : IRMV_NUM_CLASSES;
    o.anchor = d.anchor;
    det_pose(d, shift, ox, oy, o);
    o.reserved = e->refined ? d.pad_ : 0;   // the refine flag (IRMV_POINTS_REFINED); every other engine: 0
    if (shift)
        for (int j = 0; j < 4; j++) o.xyxy[j] += (j & 1) ? oy : ox;
}

extern "C" int irmv_engine_results(irmv_engine *e, int slot, irmv_det *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    const DevFrameOut &fo = *e->fout.host_at(slot);
    const int k = std::min(fo.num_dets, cap);
    for (int i = 0; i < k; i++) slot_det(e, slot, i, out[i]);
    *n = k;
    return IRMV_OK;
}

extern "C" int irmv_engine_detect(irmv_engine *e, int slot, irmv_det *out, int cap, int *n)
{
    const auto t0 = std::chrono::high_resolution_clock::now();
    // a synchronous single-slot call has nothing to overlap with: upload, graph and download ride ONE stream
    TRY(irmv_engine_submit(e, slot, 1, IRMV_SUBMIT_H2D));
    TRY(irmv_engine_wait_slots(e, slot, 1));
    const int rc = irmv_engine_results(e, slot, out, cap, n);
    e->last_detect_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    return rc;
}

extern "C" double irmv_engine_last_detect_ms(const irmv_engine *e) { return e ? e->last_detect_ms : 0.0; }

// The slot's pinned frame -> the HWC device frame of its view on stream st, outside a step: an HWC engine copies it there, a
// Bayer engine copies the raw frame to its device raw slot and demosaics it; in the window view of a window engine the slot's
// window is then cut out.
int irmv::load_frame(irmv_engine *e, int slot, hipStream_t st)
{
    TRY(enqueue_upload(e, choose_upload(e, slot, 1, -1, true, false), st));   // (the copy engine, uncaptured: a band or the whole frame)
    if (e->raw_dev) {
        launch_bayer(e, slot, 1, st);
        HIP_TRY(hipGetLastError());
    }
    if (view_of(e, slot).crop) {
        launch_crop(e, Step{STEP_ONE, slot, 1}, st);
        HIP_TRY(hipGetLastError());
    }
    return IRMV_OK;
}
