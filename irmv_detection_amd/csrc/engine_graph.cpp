// The engine's graph: the .irmw blob, tensors, weight packing, and the op list with its fused stand-ins (build_engine).
#include "engine_internal.hpp"

// ---- .irmw blob ------------------------------------------------------------------
#pragma pack(push, 1)
struct BlobHeader { char magic[4]; uint32_t version, nc, nk, reg_max, n_layers, dtype, reserved; };
struct BlobLayer { char name[32]; uint32_t cin, cout, k, stride, act, pad; uint64_t w_off, b_off; };
#pragma pack(pop)

// float -> IEEE fp16 bits, round to nearest even (dequantised int8 weights are stored as the fp16 the kernels multiply with)
static uint16_t float_to_half_bits(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0u));   // inf / nan
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                          // rounds to inf
    if (x < 0x33000001u) return (uint16_t)sign;                                                        // rounds to zero
    if (x < 0x38800000u) {   // subnormal half
        const int shift = 126 - (int)(x >> 23);                     // 14..24
        const uint32_t man = (x & 0x7fffffu) | 0x800000u;
        uint32_t h = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    uint32_t h = ((x >> 23) - 112u) << 10 | ((x >> 13) & 0x3ffu);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
}

// ---- tensors, weight packing and the layer ops -----------------------------------------
// THE device allocation of an engine: every range is recorded with its name and its tag (engine_internal.hpp, MemTag), which
// the call site chooses from what the range's consumers do with its words and says so in a comment.
int irmv::dev_alloc(irmv_engine *e, void **p, size_t bytes, const std::string &name, MemTag tag)
{
    static const char *const cls[] = {"CONST", "ACT", "CARRIED", "SCRATCH"};
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    e->dev_allocs.push_back(DevRange{name, tag, *p, bytes ? bytes : 16});
    log_range(e, (std::string(cls[tag.cls]) + " " + name).c_str(), *p, bytes ? bytes : 16);
    return IRMV_OK;
}

static int new_tensor(irmv_engine *e, const std::string &name, int H, int W, int C, bool f32, int *idx)
{
    Tensor t;
    t.name = name;
    t.H = H; t.W = W; t.C = C; t.f32 = f32;
    t.slot_elems = (size_t)H * W * C;
    // an activation tensor: convs, pools and fused kernels read its halfwords as fp16 values only
    TRY(dev_alloc(e, &t.base, t.slot_elems * t.esize() * e->cfg.num_slots, name, mem_act(f32 ? MEM_F32 : MEM_F16)));
    // activations start at zero so that never-written pad channels are finite
    HIP_TRY(hipMemset(t.base, 0, t.slot_elems * t.esize() * e->cfg.num_slots));
    *idx = (int)e->tensors.size();
    e->tensor_idx[name] = *idx;
    e->tensors.push_back(t);
    return IRMV_OK;
}

static const LayerW *find_layer(const irmv_engine *e, const std::string &name)
{
    for (auto &l : e->layers)
        if (l.name == name) return &l;
    return nullptr;
}

// output channel held by row p of 16-row MFMA tile t (see k_conv.hip epilogue)
static int tile_row_cout(int t, int p, bool pair)
{
    if (!pair) return t * 16 + p;
    return (t >> 1) * 32 + (p >> 2) * 8 + (t & 1) * 4 + (p & 3);
}

static int pack_conv(irmv_engine *e, const LayerW &l, Op &op)
{
    const int taps = l.k * l.k;
    op.cout_pad = (l.cout + 15) / 16 * 16;
    const int ntiles = op.cout_pad / 16;
    const bool pair = !op.cfg.out_f32 && (op.cout_pad % 32 == 0);   // independent of the tile shape chosen later
    op.pair = pair;
    const int cpt = (l.cin + 31) / 32;
    op.ksteps = op.cfg.cin16 ? (taps + 1) / 2 : taps * cpt;
    std::vector<uint16_t> packed((size_t)ntiles * op.ksteps * 512, 0);
    for (int t = 0; t < ntiles; t++)
        for (int ks = 0; ks < op.ksteps; ks++)
            for (int lane = 0; lane < 64; lane++) {
                const int g = lane >> 4, r = lane & 15;
                const int co = tile_row_cout(t, r, pair);
                for (int j = 0; j < 8; j++) {
                    int tap, c;
                    if (op.cfg.cin16) { tap = 2 * ks + (g >> 1); c = 8 * (g & 1) + j; }
                    else { tap = ks / cpt; c = (ks % cpt) * 32 + 8 * g + j; }
                    uint16_t v = 0;
                    if (co < l.cout && tap < taps && c < l.cin) v = l.w[((size_t)co * taps + tap) * l.cin + c];
                    packed[(((size_t)t * op.ksteps + ks) * 64 + lane) * 8 + j] = v;
                }
            }
    // SiLU layers compute on log2 e-scaled activations (irmv_common.hpp, "activation scale"): weights as they are, the bias
    // scaled once here; layers without activation (the Detect finals) undo the scale in their epilogue and keep their bias
    std::vector<float> bias(op.cout_pad, 0.f);
    for (int i = 0; i < l.cout; i++) bias[i] = l.act == 1 ? (float)((double)l.b[i] * (double)kActScale) : l.b[i];
    // weights and biases: uploaded below, read as MFMA operands (names "w." / "b." + l.name)
    TRY(dev_alloc(e, (void **)&op.w_packed, packed.size() * 2, "w." + l.name, mem_const(MEM_F16)));
    TRY(dev_alloc(e, (void **)&op.bias, bias.size() * 4, "b." + l.name, mem_const(MEM_F32)));
    HIP_TRY(hipMemcpy(op.w_packed, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(op.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    if (l.k == 1 && l.cin == 16 && op.cfg.out_f32 && l.act == 0 && op.cout_pad == 16) {   // lane (g, r): output channel r, input channels 4 g .. 4 g + 3
        std::vector<uint16_t> pk(64 * 4, 0);
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++)
                if ((lane & 15) < l.cout) pk[lane * 4 + j] = l.w[(size_t)(lane & 15) * l.cin + 4 * (lane >> 4) + j];
        TRY(dev_alloc(e, (void **)&op.w_k16, pk.size() * 2, "w." + l.name + ".k16", mem_const(MEM_F16)));
        HIP_TRY(hipMemcpy(op.w_k16, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    }
    // LDS-kernel layout: [n-block][chunk of 32 ch][tap][tile in block][lane][8]
    if (l.k == 3 && l.cin % 32 == 0 && l.act == 1 && !op.cfg.out_f32) {
        const int chunks = l.cin / 32;
        for (int v = 0; v < 4; v++) {
            const int nt = 1 << v;
            if (ntiles % nt != 0 || (nt > 1 && !pair)) continue;
            if (nt == 8 && l.stride != 2) continue;      // the 128-channel workgroup exists for the stride-2 layers only (k_conv.hip)
            std::vector<uint16_t> pl((size_t)ntiles * chunks * 9 * 512, 0);
            for (int t = 0; t < ntiles; t++)
                for (int ch = 0; ch < chunks; ch++)
                    for (int tap = 0; tap < 9; tap++)
                        for (int lane = 0; lane < 64; lane++) {
                            const int g = lane >> 4, r = lane & 15;
                            const int co = tile_row_cout(t, r, pair);
                            const int nb = t / nt, ti = t % nt;
                            const size_t base = ((((size_t)nb * chunks + ch) * 9 + tap) * nt + ti) * 512 + (size_t)lane * 8;
                            for (int j = 0; j < 8; j++) {
                                const int c = ch * 32 + 8 * g + j;
                                if (co < l.cout) pl[base + j] = l.w[((size_t)co * 9 + tap) * l.cin + c];
                            }
                        }
            TRY(dev_alloc(e, (void **)&op.w_lds[v], pl.size() * 2, "w." + l.name + ".lds" + std::to_string(v), mem_const(MEM_F16)));
            HIP_TRY(hipMemcpy(op.w_lds[v], pl.data(), pl.size() * 2, hipMemcpyHostToDevice));
        }
    }
    return IRMV_OK;
}

static int add_conv(irmv_engine *e, const std::string &layer, SegRef s0, SegRef s1, int Hin, int Win, int out_t,
                    int out_coff, int res_t = -1, int res_coff = 0)
{
    const LayerW *l = find_layer(e, layer);
    if (!l) return fail(IRMV_ERR_MODEL, "weight blob has no layer " + layer);
    if (l->cin != s0.C + s1.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": cin does not match the graph");
    Op op;
    op.kind = OP_CONV;
    op.layer = layer;
    op.s0 = s0; op.s1 = s1;
    op.Hin = Hin; op.Win = Win;
    op.Hout = Hin / l->stride; op.Wout = Win / l->stride;
    op.cin = l->cin; op.cout = l->cout;
    op.out_t = out_t; op.out_coff = out_coff; op.res_t = res_t; op.res_coff = res_coff;
    const Tensor &ot = e->tensors[out_t];
    if (ot.H != op.Hout || ot.W != op.Wout) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output shape mismatch");
    const int cout_pad = (l->cout + 15) / 16 * 16;
    if (out_coff + cout_pad > ot.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output slice out of range");
    op.cfg.ks = l->k; op.cfg.stride = l->stride; op.cfg.act = l->act; op.cfg.out_f32 = ot.f32;
    op.cfg.cin16 = (l->cin == 16 && l->k == 3);
    op.cfg.lds = false;
    op.cfg.ipw = 1;
    const int nt_all = cout_pad / 16;
    op.cfg.nt = nt_all >= 4 ? 4 : nt_all;
    // enough workgroups to cover 256 CUs a few times, else halve the pixel tile
    const long m_batch = (long)e->cfg.num_slots * op.Hout * op.Wout;
    const long blocks_mt2 = ((m_batch + 127) / 128) * (cout_pad / (16 * op.cfg.nt));
    op.cfg.mt = blocks_mt2 >= 512 ? 2 : 1;
    op.cfg_one = op.cfg;
    op.cfg_one.mt = 1;
    conv_cfg_name(op.cfg, op.kname, sizeof op.kname);
    conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one);
    op.flops = 2.0 * op.Hout * op.Wout * (double)l->cout * l->cin * l->k * l->k;
    // algorithmic bytes: every input element once (a half-resolution segment = the tensor that exists, not its upsampled
    // image), the output once, the weights once
    op.bytes = 2.0 * ((double)(Hin >> s0.shift) * (Win >> s0.shift) * s0.C + (double)(Hin >> s1.shift) * (Win >> s1.shift) * s1.C) +
               (double)op.Hout * op.Wout * l->cout * (ot.f32 ? 4.0 : 2.0) + 2.0 * l->cout * l->cin * l->k * l->k;
    op.w_bytes = 2.0 * l->cout * l->cin * l->k * l->k;
    op.out_bytes = (double)op.Hout * op.Wout * l->cout * (ot.f32 ? 4.0 : 2.0);
    TRY(pack_conv(e, *l, op));
    e->ops.push_back(op);
    return IRMV_OK;
}

// Depthwise 3x3 (ShuffleNetV2 stages): weights repacked tap-major [9][C] so that a lane's 8 channels are one 16-byte load
static int add_dw(irmv_engine *e, const std::string &layer, SegRef in, int Hin, int Win, int out_t, int out_coff)
{
    const LayerW *l = find_layer(e, layer);
    if (!l) return fail(IRMV_ERR_MODEL, "weight blob has no layer " + layer);
    if (l->groups != l->cout || l->cout != in.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": not a depthwise conv over the graph's channels");
    Op op;
    op.kind = OP_DW;
    op.layer = layer;
    op.s0 = in;
    op.Hin = Hin; op.Win = Win; op.Hout = Hin / l->stride; op.Wout = Win / l->stride;
    op.cin = op.cout = op.cout_pad = l->cout;
    op.cfg.stride = l->stride;
    op.out_t = out_t; op.out_coff = out_coff;
    const Tensor &ot = e->tensors[out_t];
    if (ot.H != op.Hout || ot.W != op.Wout || out_coff + l->cout > ot.C) return fail(IRMV_ERR_MODEL, "layer " + layer + ": output shape mismatch");
    std::vector<uint16_t> w((size_t)9 * l->cout);
    for (int c = 0; c < l->cout; c++)
        for (int t = 0; t < 9; t++) w[(size_t)t * l->cout + c] = l->w[(size_t)c * 9 + t];
    TRY(dev_alloc(e, (void **)&op.w_packed, w.size() * 2, "w." + layer, mem_const(MEM_F16)));
    TRY(dev_alloc(e, (void **)&op.bias, (size_t)l->cout * 4, "b." + layer, mem_const(MEM_F32)));
    HIP_TRY(hipMemcpy(op.w_packed, w.data(), w.size() * 2, hipMemcpyHostToDevice));
    {   // no activation, but the output feeds further layers: it stays at the activation scale, so the bias is scaled too
        std::vector<float> bs((size_t)l->cout);
        for (int i = 0; i < l->cout; i++) bs[i] = (float)((double)l->b[i] * (double)kActScale);
        HIP_TRY(hipMemcpy(op.bias, bs.data(), bs.size() * 4, hipMemcpyHostToDevice));
    }
    snprintf(op.kname, sizeof op.kname, "dwconv3x3s%d", l->stride);
    op.flops = 2.0 * op.Hout * op.Wout * (double)l->cout * 9;
    op.bytes = 2.0 * ((double)Hin * Win + (double)op.Hout * op.Wout) * l->cout + 2.0 * 9 * l->cout;
    e->ops.push_back(op);
    return IRMV_OK;
}

// concat + channel shuffle (two groups) of two bc-channel slices: out[2 i] = a[i], out[2 i + 1] = b[i]
static int add_shuffle(irmv_engine *e, const std::string &name, SegRef a, SegRef b, int H, int W, int out_t)
{
    const Tensor &ot = e->tensors[out_t];
    if (a.C != b.C || a.C % 4 != 0 || ot.C != 2 * a.C || ot.H != H || ot.W != W) return fail(IRMV_ERR_MODEL, name + ": shuffle shapes do not match");
    Op op;
    op.kind = OP_SHUF;
    op.layer = name;
    op.s0 = a; op.s1 = b;
    op.Hin = op.Hout = H; op.Win = op.Wout = W;
    op.cin = op.cout = 2 * a.C;
    op.out_t = out_t;
    snprintf(op.kname, sizeof op.kname, "shuffle_cat");
    op.bytes = 2.0 * 2.0 * (double)H * W * 2 * a.C;
    e->ops.push_back(op);
    return IRMV_OK;
}

// ShuffleNetV2 blocks (irmv_detection_amd/arch.py _shuffle_down / _shuffle_unit; the oracle's shuffle_down / shuffle_unit)
static int add_shuffle_down(irmv_engine *e, const std::string &prefix, int in_t, int c1, int H, int W, int c2, int out_t)
{
    const int bc = c2 / 2, Ho = H / 2, Wo = W / 2;
    int d1, b1, p1, d2, b2;
    TRY(new_tensor(e, prefix + ".b1.dw", Ho, Wo, c1, false, &d1));
    TRY(new_tensor(e, prefix + ".b1", Ho, Wo, bc, false, &b1));
    TRY(new_tensor(e, prefix + ".b2.pw1", H, W, bc, false, &p1));
    TRY(new_tensor(e, prefix + ".b2.dw", Ho, Wo, bc, false, &d2));
    TRY(new_tensor(e, prefix + ".b2", Ho, Wo, bc, false, &b2));
    TRY(add_dw(e, prefix + ".b1.dw", SegRef{in_t, 0, c1, 0}, H, W, d1, 0));
    TRY(add_conv(e, prefix + ".b1.pw", SegRef{d1, 0, c1, 0}, SegRef{}, Ho, Wo, b1, 0));
    TRY(add_conv(e, prefix + ".b2.pw1", SegRef{in_t, 0, c1, 0}, SegRef{}, H, W, p1, 0));
    TRY(add_dw(e, prefix + ".b2.dw", SegRef{p1, 0, bc, 0}, H, W, d2, 0));
    TRY(add_conv(e, prefix + ".b2.pw2", SegRef{d2, 0, bc, 0}, SegRef{}, Ho, Wo, b2, 0));
    return add_shuffle(e, prefix + ".shuffle", SegRef{b1, 0, bc, 0}, SegRef{b2, 0, bc, 0}, Ho, Wo, out_t);
}

static int add_shuffle_unit(irmv_engine *e, const std::string &prefix, int in_t, int c, int H, int W, int out_t)
{
    const int bc = c / 2;
    int p1, d2, b2;
    TRY(new_tensor(e, prefix + ".b2.pw1", H, W, bc, false, &p1));
    TRY(new_tensor(e, prefix + ".b2.dw", H, W, bc, false, &d2));
    TRY(new_tensor(e, prefix + ".b2", H, W, bc, false, &b2));
    TRY(add_conv(e, prefix + ".b2.pw1", SegRef{in_t, bc, bc, 0}, SegRef{}, H, W, p1, 0));
    TRY(add_dw(e, prefix + ".b2.dw", SegRef{p1, 0, bc, 0}, H, W, d2, 0));
    TRY(add_conv(e, prefix + ".b2.pw2", SegRef{d2, 0, bc, 0}, SegRef{}, H, W, b2, 0));
    return add_shuffle(e, prefix + ".shuffle", SegRef{in_t, 0, bc, 0}, SegRef{b2, 0, bc, 0}, H, W, out_t);
}

// A C2f block with a 32-channel hidden width (model.4 / model.15 at a 640 net) runs as fused kernels (k_c2f.hip) when its
// layers have the shapes those kernels are written for: n = 1 -> one launch, n = 2 -> two.  The layer ops stay in the
// list as `fused_away` (read-backs of the block's internal tensors run them; they are also the bit-exactness reference).
static int fuse_c2f32(irmv_engine *e, const std::string &prefix, int n, bool shortcut, int cat, int tmp, int out_t)
{
    if (!e->sw.fused_c2f) return IRMV_OK;
    const int last = (int)e->ops.size() - 1, first = last - (2 * n + 1);
    if (n < 1 || n > 2 || first < 0) return IRMV_OK;
    const Op &c1 = e->ops[first], &c2 = e->ops[last];
    bool ok = c1.cfg.ks == 1 && c1.cout == 64 && c1.pair && c1.cin % 32 == 0 && c1.s0.C % 32 == 0 && c1.cfg.act == 1 &&
              (c1.ksteps == 2 || c1.ksteps == 4 || c1.ksteps == 6) && (n == 1 || shortcut) &&
              c2.cfg.ks == 1 && c2.cout == 64 && c2.pair && c2.cin == (2 + n) * 32 && c2.ksteps == 2 + n && c2.cfg.act == 1 && !c2.cfg.out_f32;
    for (int i = first + 1; i < last && ok; i++) {
        const Op &m = e->ops[i];
        ok = m.cfg.ks == 3 && m.cfg.stride == 1 && m.cin == 32 && m.cout == 32 && m.pair && m.ksteps == 9 && m.cfg.act == 1 && !m.cfg.cin16;
    }
    if (!ok) return IRMV_OK;
    const int bH = c1.Hin, bW = c1.Win;          // (copies: the pushes below may move e->ops)
    const double c1_bytes = c1.bytes, c1_w = c1.w_bytes;
    auto make = [&](int mode, int i_cv1, int i_m1, int i_m2, int i_cv2, const char *nm) {
        Op op;
        op.kind = OP_C2F32;
        op.mode = mode;
        op.shortcut = shortcut;
        op.layer = prefix + (mode == 0 ? " (fused)" : (mode == 1 ? " (cv1+m.0)" : " (m.1+cv2)"));
        snprintf(op.kname, sizeof op.kname, "%s", nm);
        op.sub[0] = i_cv1; op.sub[1] = i_m1; op.sub[2] = i_m2; op.sub[3] = i_cv2;
        op.Hin = bH; op.Win = bW;
        op.out_t = out_t;
        op.res_t = cat;                              // the block's concat buffer
        const double px = (double)bH * bW;
        for (int k = 0; k < 4; k++)
            if (op.sub[k] >= 0) { op.flops += e->ops[op.sub[k]].flops; e->ops[op.sub[k]].fused_away = true; op.w_bytes += e->ops[op.sub[k]].w_bytes; }
        // algorithmic bytes: block input once (mode 0 / 1), concat slices written / read, block output, every fused layer's weights
        op.bytes = op.w_bytes;
        if (mode != 2) op.bytes += c1_bytes - c1_w - px * 64 * 2.0;                // cv1's inputs
        if (mode == 1) op.bytes += px * 96 * 2.0;                                   // y0 | y1 | y2 written
        if (mode == 2) op.bytes += px * 96 * 2.0;                                   // read back
        if (mode != 1) op.bytes += px * 64 * 2.0;                                   // block output
        e->ops.push_back(op);
    };
    if (n == 1) make(0, first, first + 1, first + 2, last, "c2f32_ab");
    else { make(1, first, first + 1, first + 2, -1, "c2f32_a"); make(2, -1, first + 3, first + 4, last, "c2f32_b"); }
    e->lazy_tensors.insert(e->tensors[cat].name);
    e->lazy_tensors.insert(e->tensors[tmp].name);
    return IRMV_OK;
}

// Single-frame steps: a 64-channel Bottleneck (model.6 / 12 / 18 at a 640 net) as ONE launch, the block's last one together
// with cv2 (k_bneck.hip).  The OP_BNECK ops stand behind the block's layer ops, which stay what batched steps run (and the
// bit-exactness reference); a step of one frame skips the layers and runs the fused launches instead.
static int fuse_bneck64(irmv_engine *e, const std::string &prefix, int n, bool shortcut, int cat, int out_t)
{
    if (!e->sw.bneck64 || e->backbone != 0) return IRMV_OK;
    const int last = (int)e->ops.size() - 1, first = last - (2 * n + 1);
    if (n < 1 || n > 2 || first < 0) return IRMV_OK;
    for (int i = first; i <= last; i++)
        if (e->ops[i].kind != OP_CONV) return IRMV_OK;
    const Op &c2 = e->ops[last];
    bool ok = c2.cfg.ks == 1 && c2.cout == 128 && c2.cout_pad == 128 && c2.pair && c2.cin == (2 + n) * 64 && c2.ksteps == 2 * (2 + n) && c2.cfg.act == 1 &&
              !c2.cfg.out_f32 && c2.s1.C == 0 && c2.s0.shift == 0 && c2.res_t < 0;
    for (int i = first + 1; i < last && ok; i++) {
        const Op &m = e->ops[i];
        ok = m.cfg.ks == 3 && m.cfg.stride == 1 && m.cin == 64 && m.cout == 64 && m.pair && m.ksteps == 18 && m.cfg.act == 1 && !m.cfg.cin16 && m.w_lds[0] != nullptr &&
             m.s1.C == 0 && m.s0.shift == 0;
    }
    if (!ok) return IRMV_OK;
    const int bH = c2.Hin, bW = c2.Win;
    for (int i = 0; i < n; i++) {
        const int i_m1 = first + 1 + 2 * i, i_m2 = i_m1 + 1;
        const bool with_cv2 = i == n - 1;
        Op op;
        op.kind = OP_BNECK;
        op.mode = with_cv2 ? 1 : 0;
        op.shortcut = shortcut;
        op.layer = prefix + ".m." + std::to_string(i) + (with_cv2 ? " + cv2 (one launch)" : " (one launch)");
        snprintf(op.kname, sizeof op.kname, with_cv2 ? "bneck64_b" : "bneck64_a");
        op.sub[0] = i_m1; op.sub[1] = i_m2; op.sub[2] = with_cv2 ? last : -1;
        op.Hin = op.Hout = bH; op.Win = op.Wout = bW;
        op.out_t = with_cv2 ? out_t : cat;
        op.res_t = cat;
        const double px = (double)bH * bW;
        for (int k = 0; k < 3; k++)
            if (op.sub[k] >= 0) { op.flops += e->ops[op.sub[k]].flops; op.w_bytes += e->ops[op.sub[k]].w_bytes; }
        op.bytes = op.w_bytes + px * 64 * 2.0 + (with_cv2 ? px * (64.0 * n + 128.0) * 2.0 : px * 64 * 2.0);   // y_in once; + the other concat slices and the block output, or y_next
        op.bneck = 1;
        e->ops.push_back(op);
        const int me = (int)e->ops.size() - 1;
        e->ops[i_m1].bneck = me; e->ops[i_m2].bneck = me;
        if (with_cv2) e->ops[last].bneck = me;
    }
    e->lazy_tensors.insert(e->tensors[cat].name);   // (a single-frame step leaves the last slice of the concat buffer and the bottleneck intermediate unwritten:
    return IRMV_OK;                                 //  read-backs of them run the layer ops, like the fused 32-channel blocks')
}

// The keypoint branch of a Detect level -- the last three ops: 3x3 (Cin -> 16), 3x3 (16 -> 16) carrying the final 1x1 -- as one
// launch (k_kpt.hip).  The OP_KPT3 op stands behind the layer ops; a step runs it and skips them, read-backs of the two
// intermediate tensors run the layers (they remain the bit-exactness reference, IRMV_KPT3=0 the switch).
static int fuse_kpt3(irmv_engine *e, int level)
{
    if (!e->sw.kpt3 || e->ops.size() < 3) return IRMV_OK;
    const int i2 = (int)e->ops.size() - 1, i1 = i2 - 1, i0 = i2 - 2;
    const Op &o0 = e->ops[i0], &o1 = e->ops[i1], &o2 = e->ops[i2];
    const bool ok = o0.kind == OP_CONV && o1.kind == OP_CONV && o2.kind == OP_CONV && o1.fuse_next == i2 && o1.cfg.cin16 && o2.w_k16 &&
                    o0.cfg.ks == 3 && o0.cfg.stride == 1 && o0.cfg.act == 1 && !o0.cfg.out_f32 && !o0.cfg.cin16 && o0.cout_pad == 16 && !o0.pair && o0.res_t < 0 &&
                    o0.s1.C == 0 && o0.s0.shift == 0 && o0.w_lds[0] != nullptr && kpt3_eligible(o0.cin) && o1.s0.t == o0.out_t && o1.cin == 16 && o1.ksteps == 5 &&
                    o0.Hin == o1.Hin && o0.Win == o1.Win;
    if (!ok) return IRMV_OK;
    {   // the kernel addresses the level's input through a buffer descriptor with 32-bit byte offsets
        const Tensor &xt = e->tensors[o0.s0.t];
        if ((double)e->cfg.num_slots * xt.H * xt.W * xt.C * 2.0 >= 2147483648.0) return IRMV_OK;
    }
    Op op;
    op.kind = OP_KPT3;
    op.layer = "model.22.cv4." + std::to_string(level) + " (one launch)";
    snprintf(op.kname, sizeof op.kname, "kpt3_c%d", o0.cin);
    op.sub[0] = i0; op.sub[1] = i1; op.sub[2] = i2;
    op.Hin = op.Hout = o0.Hin; op.Win = op.Wout = o0.Win;
    op.cin = o0.cin;
    op.level = level;
    op.flops = o0.flops + o1.flops + o2.flops;
    op.w_bytes = o0.w_bytes + o1.w_bytes + o2.w_bytes;
    op.out_bytes = o2.out_bytes;
    op.bytes = op.w_bytes + (o0.bytes - o0.w_bytes - o0.out_bytes) + o2.out_bytes;   // the level's input once, the head's keypoint channels once
    op.kpt3 = 1;
    e->lazy_tensors.insert(e->tensors[o0.out_t].name);
    e->lazy_tensors.insert(e->tensors[o1.out_t].name);
    e->ops.push_back(op);
    const int me = (int)e->ops.size() - 1;
    e->ops[i0].kpt3 = e->ops[i1].kpt3 = e->ops[i2].kpt3 = me;
    return IRMV_OK;
}

// The box branch of a Detect level -- the last three ops: 3x3 (Cin -> 64), 3x3 (64 -> 64) carrying the final 1x1 -- at the
// candidate anchors only, as one launch from a list (k_boxg.hip).  The OP_BOXG op stands behind the layer ops; whether a step
// runs it in their place is the plan's decision (engine_plan.cpp box_gathers: the sparse branch, IRMV_SPARSE_GATHER), read-backs
// run the layers.
static int fuse_boxg(irmv_engine *e, int level)
{
    if (e->ops.size() < 3 || e->cfg.num_slots > 1024) return IRMV_OK;
    const int i2 = (int)e->ops.size() - 1, i1 = i2 - 1, i0 = i2 - 2;
    const Op &o0 = e->ops[i0], &o1 = e->ops[i1], &o2 = e->ops[i2];
    const bool ok = o0.kind == OP_CONV && o1.kind == OP_CONV && o2.kind == OP_CONV && o1.fuse_next == i2 && o2.cout_pad == 64 && o2.w_packed &&
                    o0.cfg.ks == 3 && o0.cfg.stride == 1 && o0.cfg.act == 1 && !o0.cfg.out_f32 && o0.cout == 64 && o0.pair && o0.res_t < 0 &&
                    o0.s1.C == 0 && o0.s0.shift == 0 && o0.w_lds[2] != nullptr && box_gather_eligible(o0.cin) &&
                    o1.cfg.ks == 3 && o1.cfg.act == 1 && o1.cin == 64 && o1.s0.t == o0.out_t && o1.s0.coff == o0.out_coff && o1.s1.C == 0 && o1.s0.shift == 0 && o1.w_lds[2] != nullptr &&
                    o0.Hin == o1.Hin && o0.Win == o1.Win && o0.Hout == o0.Hin && o0.Wout == o0.Win;
    if (!ok) return IRMV_OK;
    {   // the kernel addresses the level's input through a buffer descriptor with 32-bit byte offsets
        const Tensor &xt = e->tensors[o0.s0.t];
        if ((double)e->cfg.num_slots * xt.H * xt.W * xt.C * 2.0 >= 2147483648.0) return IRMV_OK;
    }
    Op op;
    op.kind = OP_BOXG;
    op.layer = "model.22.cv2." + std::to_string(level) + ".g";
    snprintf(op.kname, sizeof op.kname, "box_gather_c%d", o0.cin);
    op.sub[0] = i0; op.sub[1] = i1; op.sub[2] = i2;
    op.Hin = op.Hout = o0.Hin; op.Win = op.Wout = o0.Win;
    op.cin = o0.cin;
    op.level = level;
    op.boxg = 1;   // (flops and bytes stay 0: both depend on the frames)
    e->ops.push_back(op);
    const int me = (int)e->ops.size() - 1;
    e->ops[i0].boxg = e->ops[i1].boxg = e->ops[i2].boxg = me;
    return IRMV_OK;
}

static int add_c2f(irmv_engine *e, const std::string &prefix, SegRef s0, SegRef s1, int H, int W, int c2, int n,
                   bool shortcut, int out_t)
{
    const int c = c2 / 2;
    int cat, tmp;
    TRY(new_tensor(e, prefix + ".cat", H, W, (2 + n) * c, false, &cat));
    TRY(new_tensor(e, prefix + ".tmp", H, W, c, false, &tmp));
    TRY(add_conv(e, prefix + ".cv1", s0, s1, H, W, cat, 0));
    for (int i = 0; i < n; i++) {
        const std::string m = prefix + ".m." + std::to_string(i);
        TRY(add_conv(e, m + ".cv1", SegRef{cat, (1 + i) * c, c, 0}, SegRef{}, H, W, tmp, 0));
        TRY(add_conv(e, m + ".cv2", SegRef{tmp, 0, c, 0}, SegRef{}, H, W, cat, (2 + i) * c, shortcut ? cat : -1,
                     (1 + i) * c));
    }
    TRY(add_conv(e, prefix + ".cv2", SegRef{cat, 0, (2 + n) * c, 0}, SegRef{}, H, W, out_t, 0));
    TRY(fuse_c2f32(e, prefix, n, shortcut, cat, tmp, out_t));
    if (c == 64) {
        TRY(fuse_bneck64(e, prefix, n, shortcut, cat, out_t));
        if (!e->ops.empty() && e->ops.back().kind == OP_BNECK) e->lazy_tensors.insert(e->tensors[tmp].name);
    }
    return IRMV_OK;
}

// ---- build_engine's phases, in the order they run.  Allocations and the ops pushed onto e->ops keep exactly this order: op
// indices are visible through irmv_engine_ops. ----
// Tensor indices of the graph's activations (SURVEY.md Appendix A numbers the layers), the tensors the neck reads, and the
// level sizes h<s> x w<s> = net_h / s x net_w / s.
struct Acts {
    int x0, a0, a1, a2, a3, a4, a5, a6, a7, a8, s9, a9, a12, a15, a16, a18, a19, a21, p3, p4, p5;
    int h2, h4, h8, h16, h32, w2, w4, w8, w16, w32;
};

static int create_streams_and_frames(irmv_engine *e)
{
    const irmv_engine_cfg &c = e->cfg;
    const int S = c.num_slots;
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    // default: batched engines replay concurrent sub-batches of ~64 frames, two to four of them; a stream per slot
    // for engines of TripleBuffer size, whose single-slot steps then overlap
    e->num_streams = c.num_streams > 0 ? c.num_streams : (c.num_slots <= 4 ? c.num_slots : std::min(4, std::max(2, (c.num_slots + 127) / 128)));   // batched: two graphs of up to 128 frames (round 3: with the
                                                                                                                                                   // weights-resident / multi-block kernels larger graphs win: 256 frames as 2 x 128 +6 % over 192 as 3 x 64)
    if (e->sw.has_streams) e->num_streams = e->sw.streams;
    e->num_streams = std::max(1, std::min({e->num_streams, 8, c.num_slots}));
    for (int i = 1; i < e->num_streams; i++) HIP_TRY(hipStreamCreateWithFlags(&e->extra_streams[i - 1], hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&e->h2d_stream, hipStreamNonBlocking));
    e->slot_owner.assign(S, nullptr);
    e->frame_bytes = (size_t)c.src_width * c.src_height * 3;
    const bool bayer = c.src_format != IRMV_SRC_HWC8;
    e->full_bytes = (size_t)e->full_w * e->full_h * 3;   // (= frame_bytes without a window)
    e->src_bytes = bayer ? (size_t)e->full_w * e->full_h : e->full_bytes;
    {
        // NUMA-local frame slots (SURVEY section 7 "hard parts": on a full node the copy engines read 8 x 14 k FPS x 3.93 MB =
        // 440 GB/s of host memory): the creating thread runs on the CPUs of the GPU's own socket and prefers its memory while
        // the slots are allocated and first touched (hipHostMallocNumaUser = "follow the caller's policy"); affinity and
        // policy are restored afterwards.  EngineSwitches::numa off: plain hipHostMallocDefault wherever the thread happens to run.
        const bool want = e->numa_node >= 0 && e->sw.numa;
        numa::ScopedNode scope(want ? e->numa_node : -1);
        const bool user = want && scope.policy();
        HIP_TRY(hipHostMalloc((void **)&e->src_host, e->src_bytes * S, user ? (hipHostMallocDefault | hipHostMallocNumaUser) : hipHostMallocDefault));
        log_range(e, "pinned src_host", e->src_host, e->src_bytes * S);
        memset(e->src_host, 0, e->src_bytes * S);   // first touch, by the bound thread
        if (hipHostGetDevicePointer((void **)&e->src_host_dev, e->src_host, 0) != hipSuccess) { e->src_host_dev = nullptr; (void)hipGetLastError(); }
        e->numa_placed = user && scope.bound();
    }
    // Device frames: pixel bytes.  Every consumer (preprocess / front taps, crop, demosaic and its [3][256] ISP table, light
    // extraction's threshold, metering's 256-bin histograms, render) uses a byte as a value or as an index into a table of 256
    // entries, so every byte value is valid everywhere.  SCRATCH: the upload, the crop or the demosaic writes a frame first.
    TRY(dev_alloc(e, (void **)&e->src_dev, e->frame_bytes * S, "src_dev", mem_scratch(MEM_U8)));
    HIP_TRY(hipMemset(e->src_dev, 0, e->frame_bytes * S));
    View &v0 = e->views[IRMV_VIEW_WINDOW];
    v0.built = true; v0.crop = e->window;
    v0.src_w = c.src_width; v0.src_h = c.src_height;
    v0.frames = e->src_dev; v0.frame_bytes = e->frame_bytes;
    TRY(dev_alloc(e, (void **)&v0.rot_dev, e->frame_bytes, "rot_dev", mem_scratch(MEM_U8)));   // rotate180 writes it, a D2H copy reads it
    e->slot_view.assign(S, IRMV_VIEW_WINDOW);
    e->sub_view = e->slot_view;
    if (e->window) {
        TRY(dev_alloc(e, (void **)&e->full_dev, e->full_bytes * S, "full_dev", mem_scratch(MEM_U8)));
        HIP_TRY(hipMemset(e->full_dev, 0, e->full_bytes * S));
        // the windows' corners: written by the host alone (write_window); window_crop_kernel, tile_merge_kernel and the meter
        // clamp what they read
        TRY(dev_alloc(e, (void **)&e->win_dev, sizeof(int2) * S, "win_dev", mem_const(MEM_INDEX)));
    }
    if (bayer) {
        TRY(dev_alloc(e, (void **)&e->raw_dev, e->src_bytes * S, "raw_dev", mem_scratch(MEM_U8)));
        HIP_TRY(hipMemset(e->raw_dev, 0, e->src_bytes * S));
        // phase of the R sites: IRMV_SRC_BAYER_{RGGB, BGGR, GRBG, GBRG}8 -> R at (0,0), (1,1), (0,1), (1,0)
        static const int ry[4] = {0, 1, 0, 1}, rx[4] = {0, 1, 1, 0};
        BayerArgs &b = e->bayer;
        b.raw_slot_bytes = e->src_bytes; b.dst_slot_bytes = e->full_bytes;
        b.W = e->full_w; b.H = e->full_h;
        b.ry = ry[c.src_format - 1]; b.rx = rx[c.src_format - 1];
        for (int i = 0; i < 3; i++) b.gain[i] = c.bayer_gain_q8[i];
        for (int i = 0; i < 3; i++) e->isp_gain[i] = c.bayer_gain_q8[i];
        for (int i = 0; i < kBayerTableBytes; i++) e->isp_lut[i] = (uint8_t)(i & 255);
        TRY(dev_alloc(e, (void **)&e->isp_table_dev, kBayerTableBytes, "isp_table", mem_const(MEM_U8)));
        e->bayer_mhc = c.bayer_demosaic == IRMV_DEMOSAIC_MHC;
        if (e->bayer_mhc) { e->bayer_table = true; TRY(write_isp_table(e)); }
    }
    return IRMV_OK;
}

// preprocess, front and post geometry of a view whose source frame is src_w x src_h: front_plan, under the engine's
// environment switches, and the scale that takes net-input pixels back to that frame
int irmv::build_view_geometry(irmv_engine *e, View &v, int src_w, int src_h)
{
    const int net_w = e->cfg.net_size, net_h = e->cfg.net_height;
    irmv_engine_cfg c = e->cfg;
    c.src_width = src_w; c.src_height = src_h;
    std::vector<AxisTap> tx, ty;
    irmv_front_plan_t &plan = v.front;
    front_plan(c, e->sw.front, &plan, tx, ty);
    // tap tables: source columns / rows and weights of the resize, uploaded below
    const char *vn = &v == &e->views[IRMV_VIEW_FRAME] ? ".frame" : "";
    TRY(dev_alloc(e, (void **)&v.tap_x, net_w * sizeof(AxisTap), std::string("tap_x") + vn, mem_const(MEM_INDEX)));
    TRY(dev_alloc(e, (void **)&v.tap_y, net_h * sizeof(AxisTap), std::string("tap_y") + vn, mem_const(MEM_INDEX)));
    HIP_TRY(hipMemcpy(v.tap_x, tx.data(), net_w * sizeof(AxisTap), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v.tap_y, ty.data(), net_h * sizeof(AxisTap), hipMemcpyHostToDevice));
    v.fused_front = plan.fused != 0;
    if (!e->sw.fused_front) v.fused_front = false;
    if (v.fused_front && !front_prepare()) v.fused_front = false;
    const int px = plan.box[0], py = plan.box[2], nw = plan.box[1] - px, nh = plan.box[3] - py;   // the letterbox box
    if (c.resize_mode == IRMV_RESIZE_STRETCH) {
        v.scale_x = (float)src_w / (float)net_w;   // src/yolo_engine.cpp:155-156
        v.scale_y = (float)src_h / (float)net_h;
        v.off_x = v.off_y = 0.f;
    } else {
        v.scale_x = (float)src_w / (float)nw;
        v.scale_y = (float)src_h / (float)nh;
        v.off_x = (float)px;
        v.off_y = (float)py;
    }
    return IRMV_OK;
}

// model.1.conv has the shape the fused front kernel is written for
static bool front_takes_model1(const Op &m1) { return m1.cfg.cin16 && m1.ksteps == 5 && m1.pair && m1.cout_pad == 32 && m1.out_coff == 0; }

// the op that stands for preprocess + model.0.conv + model.1.conv in the steps of a view whose front is fused
static void add_front_op(irmv_engine *e, double frame_bytes)
{
    const Op &m1 = e->ops[e->front_ops[2]];
    const Tensor &ot = e->tensors[m1.out_t];
    Op op; op.kind = OP_FRONT; op.layer = "preprocess+model.0+model.1"; snprintf(op.kname, sizeof op.kname, "front_fused");
    op.flops = e->ops[e->front_ops[1]].flops + m1.flops;
    op.bytes = frame_bytes + (double)ot.H * ot.W * 32 * 2;
    op.w_packed = m1.w_packed; op.bias = m1.bias; op.out_t = m1.out_t;
    e->lazy_tensors.insert("input"); e->lazy_tensors.insert("0");
    e->front_op = (int)e->ops.size();
    e->ops.push_back(op);
}

// scratch of the classical extraction that grows with the view's frame: per slot a padded label image
static int alloc_view_light(irmv_engine *e, View &v)
{
    const size_t SL = (e->classical || e->refined) ? (size_t)e->cfg.num_slots : 1;   // keypoint mode keeps one slot's worth for irmv_engine_extract_armors
    v.light_pool = std::max<size_t>((size_t)8 * v.src_w * v.src_h, (size_t)(v.src_w + 2) * (v.src_h + 2) + 16);
    // light_extract_kernel thresholds every byte of an ROI's padded label image before its scan reads it; the scan and the
    // border following compare labels (0, 1, the two border marks) and never index by one
    return dev_alloc(e, (void **)&v.light_labels, SL * v.light_pool, &v == &e->views[IRMV_VIEW_FRAME] ? "light_labels.frame" : "light_labels", mem_scratch(MEM_U8));
}

// The frame view of a window engine (irmv_engine_set_view): the full frame's geometry and tap tables, the larger label pool
// and rotated-image buffer, and the launch lists.  Nothing of the engine is in flight.
int irmv::build_frame_view(irmv_engine *e)
{
    View &v = e->views[IRMV_VIEW_FRAME];
    if (v.built) return IRMV_OK;
    v.crop = false;
    v.src_w = e->full_w; v.src_h = e->full_h;
    v.frames = e->full_dev; v.frame_bytes = e->full_bytes;
    TRY(build_view_geometry(e, v, e->full_w, e->full_h));
    if (!front_takes_model1(e->ops[e->front_ops[2]])) v.fused_front = false;
    if (v.fused_front && e->front_op < 0) add_front_op(e, (double)e->frame_bytes);   // (its bytes count view 0's frame; build_step_plans adds the difference)
    TRY(alloc_view_light(e, v));
    TRY(dev_alloc(e, (void **)&v.rot_dev, v.frame_bytes, "rot_dev.frame", mem_scratch(MEM_U8)));
    build_step_plans(e, v);
    HIP_TRY(hipDeviceSynchronize());
    v.built = true;
    return IRMV_OK;
}

// graph: every activation tensor, then the input stage, the front and the backbone's ops
static int build_trunk(irmv_engine *e, Acts &act)
{
    const irmv_engine_cfg &c = e->cfg;
    const int net_w = c.net_size, net_h = c.net_height;
    const bool bayer = c.src_format != IRMV_SRC_HWC8;
    act.h2 = net_h / 2; act.h4 = net_h / 4; act.h8 = net_h / 8; act.h16 = net_h / 16; act.h32 = net_h / 32;
    act.w2 = net_w / 2; act.w4 = net_w / 4; act.w8 = net_w / 8; act.w16 = net_w / 16; act.w32 = net_w / 32;
    const bool shuffle = e->backbone == 1;   // ShuffleNetV2 stages: blocks 2..8, P3 / P4 / P5 = tensors "3" / "6" / "8"
    const struct { const char *name; int s, C; int *idx; } tensors[] = {   // H x W = net_h / s x net_w / s, C channels; allocated in this order
        {"input", 1, 4, &act.x0}, {"0", 2, 16, &act.a0}, {"1", 4, 32, &act.a1}, {"2", shuffle ? 8 : 4, shuffle ? 64 : 32, &act.a2}, {"3", 8, 64, &act.a3},
        {"4", shuffle ? 16 : 8, shuffle ? 128 : 64, &act.a4}, {"5", 16, 128, &act.a5}, {"6", 16, 128, &act.a6}, {"7", 32, 256, &act.a7}, {"8", 32, 256, &act.a8},
        {"9.cat", 32, 512, &act.s9}, {"9", 32, 256, &act.a9}, {"12", 16, 128, &act.a12}, {"15", 8, 64, &act.a15}, {"16", 16, 64, &act.a16},
        {"18", 16, 128, &act.a18}, {"19", 32, 128, &act.a19}, {"21", 32, 256, &act.a21}};
    for (const auto &t : tensors) TRY(new_tensor(e, t.name, net_h / t.s, net_w / t.s, t.C, false, t.idx));

    if (bayer) {   // raw slot -> src_dev: the first op of every step (not of run_post, not of a read-back's materialisation)
        Op op; op.kind = OP_DEMOSAIC; op.layer = "demosaic"; snprintf(op.kname, sizeof op.kname, "%s", demosaic_kname(e));
        op.bytes = (double)e->src_bytes + (double)e->full_bytes;
        e->ops.push_back(op);
    }
    if (e->window) {   // the slot's window -> src_dev: behind the demosaic, in front of everything else (like it, not part of run_post or a read-back)
        Op op; op.kind = OP_CROP; op.layer = "window_crop"; snprintf(op.kname, sizeof op.kname, "window_crop");
        op.bytes = 2.0 * (double)e->frame_bytes;
        e->ops.push_back(op);
    }
    e->front_ops[0] = (int)e->ops.size(); e->front_ops[1] = e->front_ops[0] + 1; e->front_ops[2] = e->front_ops[0] + 2;   // OP_PRE, OP_CONV0, model.1.conv
    { Op op; op.kind = OP_PRE; op.layer = "preprocess"; snprintf(op.kname, sizeof op.kname, "preprocess"); op.out_t = act.x0;
      op.bytes = (double)e->frame_bytes + (double)net_h * net_w * 8; e->ops.push_back(op); }
    {
        const LayerW *l = find_layer(e, "model.0.conv");
        if (!l || l->cin != 3 || l->cout != 16 || l->k != 3 || l->stride != 2)
            return fail(IRMV_ERR_MODEL, "model.0.conv missing or not 3x3 s2 3->16");
        // A fragments of the single 16-channel tile: lane (g, r) of k-step s holds channel r,
        // k = 32 s + 8 g + j  ->  kernel row kh = 2 s + (g >> 1), tap slot kw = 2 (g & 1) + (j >> 2), channel j & 3
        std::vector<uint16_t> w(2 * 64 * 8, 0);
        std::vector<float> b(16);
        for (int o = 0; o < 16; o++) b[o] = (float)((double)l->b[o] * (double)kActScale);   // (irmv_common.hpp, "activation scale")
        for (int ks = 0; ks < 2; ks++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int g = lane >> 4, o = lane & 15;
                    const int kh = 2 * ks + (g >> 1), kw = 2 * (g & 1) + (j >> 2), ci = j & 3;
                    if (kh < 3 && kw < 3 && ci < 3) w[((size_t)ks * 64 + lane) * 8 + j] = l->w[(o * 9 + kh * 3 + kw) * 3 + ci];
                }
        TRY(dev_alloc(e, (void **)&e->conv0_w, w.size() * 2, "w.conv0", mem_const(MEM_F16)));
        TRY(dev_alloc(e, (void **)&e->conv0_b, b.size() * 4, "b.conv0", mem_const(MEM_F32)));
        HIP_TRY(hipMemcpy(e->conv0_w, w.data(), w.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->conv0_b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
        Op op; op.kind = OP_CONV0; op.layer = "model.0.conv"; snprintf(op.kname, sizeof op.kname, "conv0_mfma");
        op.s0.t = act.x0; op.out_t = act.a0;
        op.flops = 2.0 * act.h2 * act.w2 * 16 * 27;
        op.bytes = (double)net_h * net_w * 8 + (double)act.h2 * act.w2 * 32 + 27 * 16 * 2;
        e->ops.push_back(op);
    }
    TRY(add_conv(e, "model.1.conv", SegRef{act.a0, 0, 16, 0}, SegRef{}, act.h2, act.w2, act.a1, 0));
    {
        View &v0 = e->views[IRMV_VIEW_WINDOW];
        if (!front_takes_model1(e->ops.back())) v0.fused_front = false;
        if (v0.fused_front) {
            for (Op &o : e->ops) o.fused_away = o.kind != OP_DEMOSAIC && o.kind != OP_CROP;   // preprocess, model.0.conv, model.1.conv
            add_front_op(e, (double)e->frame_bytes);
        }
    }
    act.p3 = act.a4; act.p4 = act.a6; act.p5 = act.a8;   // the tensors the neck reads
    if (shuffle) {
        TRY(add_shuffle_down(e, "model.2", act.a1, 32, act.h4, act.w4, 64, act.a2));
        TRY(add_shuffle_unit(e, "model.3", act.a2, 64, act.h8, act.w8, act.a3));
        TRY(add_shuffle_down(e, "model.4", act.a3, 64, act.h8, act.w8, 128, act.a4));
        TRY(add_shuffle_unit(e, "model.5", act.a4, 128, act.h16, act.w16, act.a5));
        TRY(add_shuffle_unit(e, "model.6", act.a5, 128, act.h16, act.w16, act.a6));
        TRY(add_shuffle_down(e, "model.7", act.a6, 128, act.h16, act.w16, 256, act.a7));
        TRY(add_shuffle_unit(e, "model.8", act.a7, 256, act.h32, act.w32, act.a8));
        act.p3 = act.a3;
    } else {
    TRY(add_c2f(e, "model.2", SegRef{act.a1, 0, 32, 0}, SegRef{}, act.h4, act.w4, 32, 1, true, act.a2));
    {
        // model.2 as one kernel (k_c2f.hip) when its four layers have the shapes that kernel is written for
        const int n = (int)e->ops.size();
        const Op &c1 = e->ops[n - 4], &m1 = e->ops[n - 3], &m2 = e->ops[n - 2], &c2 = e->ops[n - 1];
        bool ok = c1.cin == 32 && c1.cout == 32 && c1.cfg.ks == 1 && c1.pair && c1.ksteps == 1 &&
                  m1.cin == 16 && m1.cout == 16 && m1.cfg.cin16 && m1.ksteps == 5 && !m1.pair &&
                  m2.cin == 16 && m2.cout == 16 && m2.cfg.cin16 && m2.ksteps == 5 && !m2.pair && m2.res_t >= 0 &&
                  c2.cin == 48 && c2.cout == 32 && c2.cfg.ks == 1 && c2.pair && c2.ksteps == 2 &&
                  c1.cfg.act == 1 && m1.cfg.act == 1 && m2.cfg.act == 1 && c2.cfg.act == 1;
        if (!e->sw.fused_c2f) ok = false;
        if (ok) {
            Op op; op.kind = OP_C2F2; op.layer = "model.2 (cv1+m.0+cv2)"; snprintf(op.kname, sizeof op.kname, "c2f2_fused");
            op.flops = c1.flops + m1.flops + m2.flops + c2.flops;
            op.bytes = 2.0 * (double)act.h4 * act.w4 * 32 * 2;
            for (int i = 0; i < 4; i++) { op.sub[i] = n - 4 + i; e->ops[n - 4 + i].fused_away = true; }
            op.s0 = c1.s0; op.out_t = c2.out_t;
            e->lazy_tensors.insert("model.2.cat"); e->lazy_tensors.insert("model.2.tmp");
            e->ops.push_back(op);
        }
    }
    TRY(add_conv(e, "model.3.conv", SegRef{act.a2, 0, 32, 0}, SegRef{}, act.h4, act.w4, act.a3, 0));
    TRY(add_c2f(e, "model.4", SegRef{act.a3, 0, 64, 0}, SegRef{}, act.h8, act.w8, 64, 2, true, act.a4));
    TRY(add_conv(e, "model.5.conv", SegRef{act.a4, 0, 64, 0}, SegRef{}, act.h8, act.w8, act.a5, 0));
    TRY(add_c2f(e, "model.6", SegRef{act.a5, 0, 128, 0}, SegRef{}, act.h16, act.w16, 128, 2, true, act.a6));
    TRY(add_conv(e, "model.7.conv", SegRef{act.a6, 0, 128, 0}, SegRef{}, act.h16, act.w16, act.a7, 0));
    TRY(add_c2f(e, "model.8", SegRef{act.a7, 0, 256, 0}, SegRef{}, act.h32, act.w32, 256, 1, true, act.a8));
    }
    return IRMV_OK;
}

// the neck, then the Detect head
static int build_neck_and_head(irmv_engine *e, const Acts &act)
{
    const int S = e->cfg.num_slots;
    TRY(add_conv(e, "model.9.cv1", SegRef{act.p5, 0, 256, 0}, SegRef{}, act.h32, act.w32, act.s9, 0));
    { Op op; op.kind = OP_POOL; op.layer = "model.9.m"; snprintf(op.kname, sizeof op.kname, "sppf_pool"); op.out_t = act.s9;
      op.bytes = (double)act.h32 * act.w32 * 128 * 2 * 4; e->ops.push_back(op); }
    TRY(add_conv(e, "model.9.cv2", SegRef{act.s9, 0, 512, 0}, SegRef{}, act.h32, act.w32, act.a9, 0));
    TRY(add_c2f(e, "model.12", SegRef{act.a9, 0, 256, 1}, SegRef{act.p4, 0, 128, 0}, act.h16, act.w16, 128, 1, false, act.a12));
    TRY(add_c2f(e, "model.15", SegRef{act.a12, 0, 128, 1}, SegRef{act.p3, 0, 64, 0}, act.h8, act.w8, 64, 1, false, act.a15));
    TRY(add_conv(e, "model.16.conv", SegRef{act.a15, 0, 64, 0}, SegRef{}, act.h8, act.w8, act.a16, 0));
    TRY(add_c2f(e, "model.18", SegRef{act.a16, 0, 64, 0}, SegRef{act.a12, 0, 128, 0}, act.h16, act.w16, 128, 1, false, act.a18));
    TRY(add_conv(e, "model.19.conv", SegRef{act.a18, 0, 128, 0}, SegRef{}, act.h16, act.w16, act.a19, 0));
    TRY(add_c2f(e, "model.21", SegRef{act.a19, 0, 128, 0}, SegRef{act.a9, 0, 256, 0}, act.h32, act.w32, 256, 1, false, act.a21));

    // Detect head: per level one fp32 record of kHeadRec per anchor: box 64 | cls 16 | kpt 16
    const int P[3] = {act.a15, act.a18, act.a21}, PC[3] = {64, 128, 256}, PH[3] = {act.h8, act.h16, act.h32}, PW[3] = {act.w8, act.w16, act.w32};
    int base = 0;
    for (int i = 0; i < 3; i++) {
        e->lvl_hw[i] = PH[i] * PW[i];
        e->lvl_base[i] = base;
        base += e->lvl_hw[i];
    }
    e->A = base;
    // the head records: fp32 logits, read as values by the scan, the DFL decode and the keypoint decode
    TRY(dev_alloc(e, (void **)&e->head_all, (size_t)S * e->A * kHeadRec * 4, "head_all", mem_act(MEM_F32)));
    HIP_TRY(hipMemset(e->head_all, 0, (size_t)S * e->A * kHeadRec * 4));
    for (int i = 0; i < 3; i++) {   // per-level views [slot][H*W][kHeadRec] into the one head allocation
        Tensor t;
        t.name = "head." + std::to_string(i);
        t.H = PH[i]; t.W = PW[i]; t.C = kHeadRec; t.f32 = true;
        t.slot_elems = (size_t)PH[i] * PW[i] * kHeadRec;
        t.base = e->head_all + (size_t)e->lvl_base[i] * S * kHeadRec;
        e->head_t[i] = (int)e->tensors.size();
        e->tensor_idx[t.name] = e->head_t[i];
        e->tensors.push_back(t);
    }
    const char *br[3] = {"cv2", "cv3", "cv4"};
    const int mid[3] = {64, 64, 16}, off[3] = {0, kClsOff, kKptOff};
    const int nbr = e->nk > 0 ? 3 : 2;
    // Engines that never batch (every step is a single frame: the reference node's shape) run the first-stage 3x3 convs of a
    // level's branches -- same input, 64 + 64 (+ 16) output channels -- as ONE conv: the weights are concatenated along
    // cout (keypoint branch padded to 32 channels with zeros), the second-stage convs read channel slices of the merged
    // output.  Same K order per output channel -> same bits; two or three launches fewer per level, and the level's input
    // is staged once.  Batched engines keep the separate convs (their nt = 4 tiles do not divide 160 channels).
    {
        e->merge_head0 = e->sw.merge_head0 == 1 || (e->sw.merge_head0 != 0 && stream_share(e, S) == 1);
        for (int i = 0; i < 3 && e->merge_head0; i++)          // every branch conv must have the shape the merge assumes
            for (int b = 0; b < nbr; b++) {
                const LayerW *l0 = find_layer(e, std::string("model.22.") + br[b] + "." + std::to_string(i) + ".0");
                if (!l0 || l0->k != 3 || l0->stride != 1 || l0->act != 1 || l0->cin != PC[i] || l0->cout != mid[b]) e->merge_head0 = false;
            }
    }
    const int coff0[3] = {0, 64, 128};
    int t_s0[3] = {-1, -1, -1};
    if (e->merge_head0) {
        const int cm = nbr == 3 ? 160 : 128;
        e->merged_w.reserve(3); e->merged_b.reserve(3);
        e->layers.reserve(e->layers.size() + 3);      // LayerW pointers handed out below stay valid
        for (int i = 0; i < 3; i++) {
            const LayerW *src[3] = {nullptr, nullptr, nullptr};
            for (int b = 0; b < nbr; b++) src[b] = find_layer(e, std::string("model.22.") + br[b] + "." + std::to_string(i) + ".0");
            const size_t per_out = (size_t)9 * PC[i];
            e->merged_w.emplace_back((size_t)cm * per_out, (uint16_t)0);
            e->merged_b.emplace_back((size_t)cm, 0.f);
            for (int b = 0; b < nbr; b++) {
                memcpy(e->merged_w.back().data() + (size_t)coff0[b] * per_out, src[b]->w, (size_t)mid[b] * per_out * 2);
                memcpy(e->merged_b.back().data() + coff0[b], src[b]->b, (size_t)mid[b] * 4);
            }
            LayerW m;
            m.name = "model.22.s0." + std::to_string(i);
            m.cin = PC[i]; m.cout = cm; m.k = 3; m.stride = 1; m.act = 1;
            m.w = e->merged_w.back().data(); m.b = e->merged_b.back().data();
            e->layers.push_back(m);
            TRY(new_tensor(e, "22.s0." + std::to_string(i), PH[i], PW[i], cm, false, &t_s0[i]));
            TRY(add_conv(e, m.name, SegRef{P[i], 0, PC[i], 0}, SegRef{}, PH[i], PW[i], t_s0[i], 0));
            Op &mo = e->ops.back();
            const double real = nbr == 3 ? 144.0 : 128.0;
            mo.flops *= real / cm;                      // algorithmic work: the zero-padded channels do not count
            mo.level = i;
        }
    }
    for (int b = 0; b < nbr; b++)
        for (int i = 0; i < 3; i++) {
            const std::string pre = std::string("model.22.") + br[b] + "." + std::to_string(i);
            const std::string tn = std::string("22.") + br[b] + "." + std::to_string(i);
            int t1 = -1, t2;
            TRY(new_tensor(e, tn + ".1", PH[i], PW[i], mid[b], false, &t2));
            if (e->merge_head0) {
                TRY(add_conv(e, pre + ".1", SegRef{t_s0[i], coff0[b], mid[b], 0}, SegRef{}, PH[i], PW[i], t2, 0));
            } else {
                TRY(new_tensor(e, tn + ".0", PH[i], PW[i], mid[b], false, &t1));
                TRY(add_conv(e, pre + ".0", SegRef{P[i], 0, PC[i], 0}, SegRef{}, PH[i], PW[i], t1, 0));
                TRY(add_conv(e, pre + ".1", SegRef{t1, 0, mid[b], 0}, SegRef{}, PH[i], PW[i], t2, 0));
            }
            TRY(add_conv(e, pre + ".2", SegRef{t2, 0, mid[b], 0}, SegRef{}, PH[i], PW[i], e->head_t[i], off[b]));
            for (size_t k = e->ops.size() - (e->merge_head0 ? 2 : 3); k < e->ops.size(); k++) e->ops[k].level = i;
            {   // the branch's final 1x1 can ride in the epilogue of its second 3x3 (k_conv.hip, N2 > 0)
                const int i1 = (int)e->ops.size() - 2, i2 = i1 + 1;
                const Op &o1 = e->ops[i1], &o2 = e->ops[i2];
                if (e->sw.fused_head && o1.cout == 64 && o1.cin % 32 == 0 && o1.pair && o1.res_t < 0 && o1.cfg.stride == 1 &&
                    o2.cin == 64 && o2.ksteps == 2 && o2.cfg.ks == 1 && o2.cfg.out_f32 && o2.cfg.act == 0 && (o2.cout_pad == 16 || o2.cout_pad == 64))
                    e->ops[i1].fuse_next = i2;
                // ... and the keypoint branch's 16 -> nk final in the epilogue of the Cin = 16 direct kernel (one 16x16x16 MFMA per 16 pixels)
                if (e->sw.fused_head && o1.cfg.cin16 && o1.cout_pad == 16 && !o1.pair && o1.res_t < 0 && o1.cfg.stride == 1 && o1.cfg.act == 1 && o2.w_k16)
                    e->ops[i1].fuse_next = i2;
            }
            if (b == 2 && !e->merge_head0) TRY(fuse_kpt3(e, i));
            if (b == 0 && !e->merge_head0) TRY(fuse_boxg(e, i));
        }
    return IRMV_OK;
}

static int build_post_stage(irmv_engine *e)
{
    const irmv_engine_cfg &c = e->cfg;
    const int net_w = c.net_size, net_h = c.net_height, S = c.num_slots;
    // ---- post-processing buffers ----
    // boxes: xyxy floats of the candidate anchors, written by the decode (scan_decode_kernel / decode_keys), read as values by
    // the NMS walks at the anchors of the frame's own keys.
    TRY(dev_alloc(e, (void **)&e->boxes, (size_t)S * e->A * 16, "boxes", mem_scratch(MEM_F32)));
    // keys: (orderable logit) << 32 | (0xffffffff - id), id = anchor * nc + class.  The low word is an INDEX: unpack_key
    // (k_post.hip) turns it into the anchor that addresses boxes and head records, clamped by anchor_of to A - 1 whatever the
    // word holds; take_keys clamps the count it reads the list to.  Valid low words are [0xffffffff - (A nc - 1), 0xffffffff],
    // so the largest valid word is 0xffffffff (id 0); the high word is a score, any value.
    TRY(dev_alloc(e, (void **)&e->keys, (size_t)S * e->A * e->nc * 8, "keys", mem_scratch_index(0xffffffffu)));
    // per-slot candidate counters of the split scan (k_post.hip scan_decode_kernel): zeroed HERE, once, with a synchronous
    // memset -- afterwards each nms_pnp launch reads its frames' counters and resets them itself (no memset node in a
    // captured step, nothing left non-zero between steps)
    if (e->sw.split_scan) {
        // CARRIED, invariant: zero between steps.  A count: the emitting epilogues and scan_decode_kernel refuse an index at or
        // above key_cap = A nc, take_keys clamps what it reads to [0, key_cap]
        TRY(dev_alloc(e, (void **)&e->cand_counts, (size_t)S * sizeof(int), "cand_counts", mem_carried_index((uint32_t)(e->A * e->nc))));
        HIP_TRY(hipMemset(e->cand_counts, 0, (size_t)S * sizeof(int)));
        // ... and the candidate-anchor bitmap of the sparse head, kept the same way
        e->cand_words = (e->A + 31) / 32;
        // CARRIED, invariant: zero between steps.  Bit masks (any word is in range; a set bit stores or computes a head row)
        TRY(dev_alloc(e, (void **)&e->cand_bits, (size_t)S * e->cand_words * sizeof(unsigned int), "cand_bits", mem_carried_index(0xffffffffu)));
        HIP_TRY(hipMemset(e->cand_bits, 0, (size_t)S * e->cand_words * sizeof(unsigned int)));
        // ... and, where a level has an OP_BOXG op, the candidate lists cand_list_kernel derives from the bitmap inside a step.
        // Indices: an entry is a pixel of its level, a count at most the level's pixels; both kernels of k_boxg.hip clamp what
        // they read to their own level, the values below are the smallest level's
        bool gathers = false;
        for (const Op &op : e->ops) gathers = gathers || op.kind == OP_BOXG;
        if (gathers) {
            TRY(dev_alloc(e, (void **)&e->boxg_list, (size_t)S * e->A * sizeof(int), "boxg_list", mem_scratch_index((uint32_t)(e->lvl_hw[2] - 1))));
            TRY(dev_alloc(e, (void **)&e->boxg_count, (size_t)3 * S * sizeof(int), "boxg_count", mem_scratch_index((uint32_t)e->lvl_hw[2])));
        }
    }
    e->head_stale.assign((size_t)S, 0);
    e->branch_stale.assign((size_t)S, 0);
    // DevDet mixes floats, doubles and int32 fields; the most dangerous use decides.  cls: light_extract_kernel and pose_rule
    // index the class tables with cls & 15 and tile_merge_kernel maps anything outside [0, 14) to 14; anchor and pnp_ok are
    // read by the host alone; armor_size (0 / 1) is the host's index into the plate sizes.  The largest word valid in every one
    // of them is 1 (0 for a model of one class).  Records at and above num_dets are read by no kernel.
    const uint32_t det_max = e->nc > 1 ? 1u : 0u;
    TRY(dev_alloc(e, (void **)&e->dets.dev, (size_t)S * c.max_det * sizeof(DevDet), "dets_dev", mem_scratch_index(det_max)));
    // num_dets is the record count of light_extract_kernel (min(n, max_det), a negative count runs nothing), refine_prior_kernel
    // and tile_merge_kernel (clamped to [0, max_det]); n_candidates (<= A nc) and the rest go to the host
    TRY(dev_alloc(e, (void **)&e->fout.dev, (size_t)S * sizeof(DevFrameOut), "fout_dev", mem_scratch_index((uint32_t)c.max_det)));
    // Result records live in mapped, coherent pinned memory: in keypoint mode the NMS kernel stores them there directly
    // (~20 KB per frame over PCIe, visible to the host once the stream is synchronised), which removes the D2H copies of
    // a step -- measured 9.6 us per synchronous call on this stack (scripts/probes/stream_probe.cpp), and copies issued
    // from the compute streams also halve the upload stream's H2D rate.  The classical mode (light_extract_kernel
    // reads and rewrites the records on the device) keeps device records + a copy.
    TRY(e->dets.pin(e, S, c.max_det, "pinned dets_host"));
    TRY(e->fout.pin(e, S, 1, "pinned fout_host"));
    // class-logit scan + box decode of the candidate anchors: kScanBlocks workgroups per frame (k_post.hip)
    if (e->sw.split_scan) {
        Op op; op.kind = OP_SCAN; op.layer = "scan_decode"; snprintf(op.kname, sizeof op.kname, "scan_decode");
        op.bytes = (double)e->A * 64.0; e->ops.push_back(op);
    }
    // [decode +] sort + NMS + keypoints + PnP: one kernel, one workgroup per frame (k_post.hip)
    { Op op; op.kind = OP_NMS; op.layer = "decode_nms_kpt_pnp"; snprintf(op.kname, sizeof op.kname, "nms_pnp");
      op.bytes = (double)e->A * 64.0; e->ops.push_back(op); }
    if (c.point_source == IRMV_POINTS_KEYPOINT_HEAD && e->nk < 8) return fail(IRMV_ERR_MODEL, "point_source = keypoint head, but the model has none");
    e->classical = c.point_source == IRMV_POINTS_CLASSICAL || (c.point_source == IRMV_POINTS_AUTO && e->nk < 8);
    e->refined = c.point_source == IRMV_POINTS_REFINED;   // (irmv_engine_create has refused a model without a keypoint head; AUTO never resolves to it)
    // the light kernel reads and rewrites the records: not across PCIe
    e->zero_copy_results = !e->classical && !e->refined && e->sw.zero_copy_results;
    if (e->classical) {
        Op op; op.kind = OP_LIGHT; op.layer = "extract_armors"; snprintf(op.kname, sizeof op.kname, "light_extract");
        e->ops.push_back(op);
    }
    if (e->refined) {   // the guided instantiation behind the NMS: the keypoints it decoded are the prior
        Op op; op.kind = OP_LIGHT; op.layer = "refine_points"; snprintf(op.kname, sizeof op.kname, "light_refine");
        e->ops.push_back(op);
        TRY(dev_alloc(e, (void **)&e->refine_dev, sizeof(RefineParams), "refine_params", mem_const(MEM_F32)));
        HIP_TRY(hipMemcpy(e->refine_dev, &e->refine, sizeof e->refine, hipMemcpyHostToDevice));
        // the prior: refine_prior_kernel copies the records' keypoints here, guided_roi range-checks all eight before use
        TRY(dev_alloc(e, (void **)&e->refine_kpts, (size_t)S * c.max_det * 8 * sizeof(float), "refine_kpts", mem_scratch(MEM_F32)));
        HIP_TRY(hipMemset(e->refine_kpts, 0, (size_t)S * c.max_det * 8 * sizeof(float)));
    }
    // scratch of the classical extraction: per detection a padded label image (ROIs up to ~510 x 510) and contour points
    const size_t SL = (e->classical || e->refined) ? (size_t)S : 1;   // keypoint mode keeps one slot's worth for irmv_engine_extract_armors
    TRY(alloc_view_light(e, e->views[IRMV_VIEW_WINDOW]));
    // contour points and hull scratch: 16-bit ROI coordinates that trace_border writes and contour_to_light sorts, hulls and
    // measures -- arithmetic only (ranks and hull indices are counted, never read from memory); s_start bounds every read
    TRY(dev_alloc(e, (void **)&e->light_points, SL * c.max_det * kLightPointsCap * 2 * sizeof(short), "light_points", mem_scratch(MEM_F16)));
    TRY(dev_alloc(e, (void **)&e->light_hulls, SL * c.max_det * kLightPointsCap * 4 * sizeof(short), "light_hulls", mem_scratch(MEM_F16)));
    // explicit boxes of irmv_engine_extract_armors, uploaded before the launch; roi_of clips them to the frame
    TRY(dev_alloc(e, (void **)&e->light_boxes, (size_t)c.max_det * 16, "light_boxes", mem_scratch(MEM_F32)));
    TRY(dev_alloc(e, (void **)&e->light_dets_dev, (size_t)c.max_det * sizeof(DevDet), "light_dets_dev", mem_scratch_index(det_max)));   // (DevDet: as dets_dev)
    HIP_TRY(hipHostMalloc((void **)&e->light_dets_host, (size_t)c.max_det * sizeof(DevDet), hipHostMallocDefault));
    log_range(e, "pinned light_dets", e->light_dets_host, (size_t)c.max_det * sizeof(DevDet));

    PostArgs &p = e->post;
    p.net_w = net_w; p.net_h = net_h; p.A = e->A; p.nc = e->nc; p.nk = e->nk;
    // class policy: uniform from cfg.score_thr / cfg.armor_size until irmv_engine_set_class_policy says otherwise
    TRY(dev_alloc(e, (void **)&e->cls_dev, 2 * sizeof(ClassTable), "cls_dev", mem_const(MEM_INDEX)));   // thresholds and plate indices, written by write_class_table
    if (int rc = irmv_class_policy_uniform(c.score_thr, c.armor_size, &e->policy)) return rc;
    TRY(write_class_table(e));
    p.cls = e->cls_dev;
    p.iou_thr = c.iou_thr;
    p.max_det = c.max_det;
    p.pre_nms_cap = c.pre_nms_cap;
    p.classwalk = e->sw.nms_classwalk ? 1 : 0;
    p.prefilter = e->sw.nms_prefilter;
    PnpConst pc;
    pc.fx = c.camera_matrix[0]; pc.fy = c.camera_matrix[4];
    pc.cx = c.camera_matrix[2]; pc.cy = c.camera_matrix[5];
    pc.k1 = c.dist_coeffs[0]; pc.k2 = c.dist_coeffs[1]; pc.p1 = c.dist_coeffs[2];
    pc.p2 = c.dist_coeffs[3]; pc.k3 = c.dist_coeffs[4];
    pc.hy[0] = 135.0 / 2.0 / 1000.0; pc.hy[1] = 225.0 / 2.0 / 1000.0;   // src/pnp_solver.cpp:18-21
    pc.hz[0] = pc.hz[1] = 55.0 / 2.0 / 1000.0;
    e->pnp_base = pc;
    TRY(dev_alloc(e, (void **)&e->pnp_dev, sizeof(PnpConst) * (e->window ? S : 1), "pnp_dev", mem_const(MEM_F64)));
    HIP_TRY(hipMemcpy(e->pnp_dev, &pc, sizeof pc, hipMemcpyHostToDevice));
    p.pnp = e->pnp_dev;
    p.pnp_stride = e->window ? 1 : 0;
    if (e->window) {   // every slot's window starts centred
        e->win_org.assign(S, int2{(e->full_w - c.src_width) / 2, (e->full_h - c.src_height) / 2});
        e->sub_org = e->win_org;
        for (int s = 0; s < S; s++) TRY(write_window(e, s));
    }
    p.dbg = nullptr;
    if (e->sw.nms_stamps) {
        TRY(dev_alloc(e, (void **)&e->dbg_dev, (size_t)S * 16 * sizeof(long long), "dbg_dev", mem_scratch(MEM_F64)));   // phase stamps: written by nms_pnp_kernel, printed by the host
        HIP_TRY(hipMemset(e->dbg_dev, 0, (size_t)S * 16 * sizeof(long long)));
        p.dbg = e->dbg_dev;
    }
    return IRMV_OK;
}

int irmv::build_engine(irmv_engine *e)
{
    HIP_TRY(hipSetDevice(e->cfg.device));
    Acts act{};
    TRY(create_streams_and_frames(e));
    TRY(build_view_geometry(e, e->views[IRMV_VIEW_WINDOW], e->cfg.src_width, e->cfg.src_height));
    TRY(build_trunk(e, act));
    TRY(build_neck_and_head(e, act));
    TRY(build_post_stage(e));
    HIP_TRY(hipDeviceSynchronize());
    return IRMV_OK;
}

int irmv::load_blob(irmv_engine *e)
{
    const irmv_engine_cfg &c = e->cfg;
    if (c.weights_path) {
        std::string path = c.weights_path;
        const size_t dot = path.find_last_of('.');
        if (dot != std::string::npos && path.substr(dot) != ".irmw") path = path.substr(0, dot) + ".irmw";
        std::ifstream f(path, std::ios::binary);
        if (!f) return fail(IRMV_ERR_MODEL, "cannot open weight blob " + path + " (convert the model to .irmw first)");
        f.seekg(0, std::ios::end);
        const size_t n = (size_t)f.tellg();
        f.seekg(0, std::ios::beg);
        e->blob.resize(n);
        f.read(reinterpret_cast<char *>(e->blob.data()), (std::streamsize)n);
    } else if (c.weights_blob && c.weights_bytes) {
        e->blob.resize(c.weights_bytes);
        if (c.weights_on_device) {
            HIP_TRY(hipSetDevice(c.device));
            HIP_TRY(hipMemcpy(e->blob.data(), c.weights_blob, c.weights_bytes, hipMemcpyDeviceToHost));
        } else {
            memcpy(e->blob.data(), c.weights_blob, c.weights_bytes);
        }
    } else {
        return fail(IRMV_ERR_MODEL, "no weights: set weights_path or weights_blob");
    }
    if (e->blob.size() < sizeof(BlobHeader)) return fail(IRMV_ERR_MODEL, "weight blob truncated");
    BlobHeader h;
    memcpy(&h, e->blob.data(), sizeof h);
    // dtype 1: fp16 weights.  dtype 2 (BASELINE configs[4], "int8 weights"): int8 OHWI weights + fp32 per-output-channel
    // scales; expanded here, once, to w = fp16(q * scale) -- the fragment packing below is dtype-agnostic from there on.
    if (memcmp(h.magic, "IRMW", 4) != 0 || h.version != 1 || (h.dtype != 1 && h.dtype != 2) || h.reg_max != 16)
        return fail(IRMV_ERR_MODEL, "not an IRMW v1 blob (fp16 or int8 weights)");
    e->dequant.reserve(h.n_layers);
    if (h.nc < 1 || h.nc > 16 || (h.nk != 0 && h.nk != 8))
        return fail(IRMV_ERR_MODEL, "unsupported head: nc must be 1..16, nk 0 or 8");
    if (h.reserved > 1) return fail(IRMV_ERR_MODEL, "unknown backbone id in the weight blob");
    e->backbone = (int)h.reserved;
    e->nc = (int)h.nc;
    e->nk = (int)h.nk;
    e->no = 64 + e->nc + e->nk;
    if (sizeof h + (size_t)h.n_layers * sizeof(BlobLayer) > e->blob.size()) return fail(IRMV_ERR_MODEL, "layer table truncated");
    for (uint32_t i = 0; i < h.n_layers; i++) {
        BlobLayer bl;
        memcpy(&bl, e->blob.data() + sizeof h + (size_t)i * sizeof bl, sizeof bl);
        LayerW l;
        char nm[33];
        memcpy(nm, bl.name, 32);
        nm[32] = 0;
        l.name = nm;
        l.cin = bl.cin; l.cout = bl.cout; l.k = bl.k; l.stride = bl.stride; l.act = bl.act;
        l.groups = bl.pad > 1 ? (int)bl.pad : 1;
        if (l.groups > 1 && !(l.groups == l.cout && l.cin == 1 && l.k == 3 && l.cout % 8 == 0 && l.act == 0))
            return fail(IRMV_ERR_MODEL, "layer " + l.name + ": only depthwise 3x3 grouped convs (no activation) are supported");
        const size_t nw = (size_t)l.cout * l.k * l.k * l.cin;
        const size_t w_bytes = h.dtype == 2 ? ((nw + 3) & ~(size_t)3) + (size_t)l.cout * 4 : nw * 2;
        if (bl.w_off + w_bytes > e->blob.size() || bl.b_off + (size_t)l.cout * 4 > e->blob.size())
            return fail(IRMV_ERR_MODEL, "layer " + l.name + " data out of range");
        l.w = reinterpret_cast<const uint16_t *>(e->blob.data() + bl.w_off);
        if (h.dtype == 2) {
            const int8_t *q = reinterpret_cast<const int8_t *>(e->blob.data() + bl.w_off);
            const float *scale = reinterpret_cast<const float *>(e->blob.data() + bl.w_off + ((nw + 3) & ~(size_t)3));
            e->dequant.emplace_back(nw);
            std::vector<uint16_t> &d = e->dequant.back();
            const size_t per_out = nw / l.cout;
            for (int o = 0; o < l.cout; o++)
                for (size_t i = 0; i < per_out; i++) d[o * per_out + i] = float_to_half_bits((float)q[o * per_out + i] * scale[o]);
            l.w = d.data();   // (the vectors were reserved above: no reallocation moves them)
        }
        l.b = reinterpret_cast<const float *>(e->blob.data() + bl.b_off);
        e->layers.push_back(l);
    }
    return IRMV_OK;
}
