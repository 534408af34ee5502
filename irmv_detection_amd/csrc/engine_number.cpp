// Plate numbers (include/irmv_hip.h, "plate numbers"; k_number.hip): the model's checks, its .irmn file, the rounding and the
// k-major upload, the switch that puts the op into the engine's steps, the step's launch, the records' way to the caller, the
// on-demand call on explicit patch records and the host softmax.  Compiled with -ffp-contract=off like the kernel's module;
// the host does no arithmetic of the model but the rounding of a weight to fp16.
#include "engine_internal.hpp"

static_assert(sizeof(DevNumber) == sizeof(irmv_plate_number) && sizeof(irmv_plate_number) == 96 && sizeof(DevNumber) == 4 * kNumRecWords &&
                  offsetof(DevNumber, state) == offsetof(irmv_plate_number, state) && offsetof(DevNumber, ones) == offsetof(irmv_plate_number, ones) &&
                  offsetof(DevNumber, margin) == offsetof(irmv_plate_number, margin) && offsetof(DevNumber, logits) == offsetof(irmv_plate_number, logits),
              "DevNumber is irmv_plate_number");
static_assert(kNumIn == IRMV_PATCH_W * IRMV_PATCH_H && kNumClassMax == IRMV_NUM_CLASSES_MAX && kNumRecWords <= 64, "header and kernel disagree");
static_assert(kNumHiddenMax <= 128 && kNumClassMax <= 64, "a lane is at most two hidden units and one logit");

constexpr float kNumValueMax = 65504.0f;
constexpr int64_t kNumFileFloatsMax = (int64_t)kNumWeightHalves + kNumBiasFloats;
constexpr size_t kNumFileHeader = 32;

// float -> IEEE fp16 bits, round to nearest even; |f| <= 65504 and finite (check_number_model)
static uint16_t number_half_bits(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x < 0x33000001u) return (uint16_t)sign;             // rounds to zero
    if (x < 0x38800000u) {                                  // subnormal half
        const int shift = 126 - (int)(x >> 23);             // 14 .. 24
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

static int check_number_shape(int n_layers, const int32_t *dims, int input, const char *who)
{
    const std::string w(who);
    if (n_layers < 1 || n_layers > kNumLayersMax) return fail(IRMV_ERR_ARG, w + ": n_layers must be 1 .. 3");
    if (dims[0] != kNumIn) return fail(IRMV_ERR_ARG, w + ": dims[0] must be 560");
    for (int l = 1; l < n_layers; l++)
        if (dims[l] < 1 || dims[l] > kNumHiddenMax) return fail(IRMV_ERR_ARG, w + ": a hidden width must be 1 .. 128");
    if (dims[n_layers] < 1 || dims[n_layers] > kNumClassMax) return fail(IRMV_ERR_ARG, w + ": the last width must be 1 .. 16");
    for (int l = n_layers + 1; l < 4; l++)
        if (dims[l] != 0) return fail(IRMV_ERR_ARG, w + ": dims behind the last layer must be 0");
    if (input != IRMV_NUM_IN_BINARY && input != IRMV_NUM_IN_GRAY) return fail(IRMV_ERR_ARG, w + ": input must be IRMV_NUM_IN_BINARY or IRMV_NUM_IN_GRAY");
    return IRMV_OK;
}

static int check_number_model(const irmv_number_model *m)
{
    if (!m) return fail(IRMV_ERR_ARG, "number model: model is null");
    if (m->struct_size != sizeof(irmv_number_model)) return fail(IRMV_ERR_ARG, "number model: struct_size is not sizeof(irmv_number_model)");
    TRY(check_number_shape(m->n_layers, m->dims, m->input, "number model"));
    for (int l = 0; l < m->n_layers; l++) {
        if (!m->weight[l] || !m->bias[l]) return fail(IRMV_ERR_ARG, "number model: a layer's weight / bias is null");
        const size_t nw = (size_t)m->dims[l] * m->dims[l + 1];
        for (size_t i = 0; i < nw; i++)
            if (!(std::fabs(m->weight[l][i]) <= kNumValueMax)) return fail(IRMV_ERR_ARG, "number model: a weight is not finite or above 65504 in magnitude");   // (a NaN fails)
        for (int i = 0; i < m->dims[l + 1]; i++)
            if (!(std::fabs(m->bias[l][i]) <= kNumValueMax)) return fail(IRMV_ERR_ARG, "number model: a bias is not finite or above 65504 in magnitude");
    }
    return IRMV_OK;
}

// e->number_table -> its device copy.  The caller has made sure that no step in flight reads it.
static int write_number_table(irmv_engine *e)
{
    e->number_table.enable = e->number_opts.enable;
    HIP_TRY(hipMemcpy(e->number_table_dev, &e->number_table, sizeof(NumberTable), hipMemcpyHostToDevice));
    return IRMV_OK;
}

extern "C" int irmv_engine_set_number_model(irmv_engine *e, const irmv_number_model *m)
{
    TRY(check_number_model(m));   // (the values first: a refused one never reaches the engine)
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));     // every stream of the engine: no step in flight reads the table or the weights
    // host-written, read when the kernel runs: widths, padded widths and offsets (all checked above) ...
    if (!e->number_table_dev) TRY(dev_alloc(e, (void **)&e->number_table_dev, sizeof(NumberTable), "number_table", mem_const(MEM_INDEX)));
    // ... the weights as fp16, k-major, sized once for the largest model, and the fp32 biases: values only
    if (!e->number_weights) TRY(dev_alloc(e, (void **)&e->number_weights, (size_t)kNumWeightHalves * sizeof(half_t), "number_weights", mem_const(MEM_F16)));
    if (!e->number_bias) TRY(dev_alloc(e, (void **)&e->number_bias, (size_t)kNumBiasFloats * sizeof(float), "number_bias", mem_const(MEM_F32)));
    NumberTable t{};
    t.n_layers = m->n_layers; t.input = m->input;
    for (int l = 0; l < 4; l++) t.dims[l] = m->dims[l];
    std::vector<uint16_t> w((size_t)kNumWeightHalves, (uint16_t)0);
    std::vector<float> b((size_t)kNumBiasFloats, 0.0f);
    int w_at = 0, b_at = 0;
    for (int l = 0; l < m->n_layers; l++) {
        const int n_in = m->dims[l], n_out = m->dims[l + 1], pad = (n_out + kNumPadUnit - 1) / kNumPadUnit * kNumPadUnit;
        t.pad[l] = pad; t.w_off[l] = w_at; t.b_off[l] = b_at;
        for (int o = 0; o < n_out; o++) {
            for (int k = 0; k < n_in; k++) w[(size_t)w_at + (size_t)k * pad + o] = number_half_bits(m->weight[l][(size_t)o * n_in + k]);
            b[(size_t)b_at + o] = m->bias[l][o];
        }
        w_at += n_in * pad; b_at += pad;
    }
    if (w_at > kNumWeightHalves || b_at > kNumBiasFloats) return fail(IRMV_ERR_ARG, "number model: larger than the largest model");   // (cannot happen within the checked widths)
    HIP_TRY(hipMemcpy(e->number_weights, w.data(), w.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->number_bias, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
    e->number_table = t;
    e->number_model = true;
    return write_number_table(e);
}

extern "C" int irmv_number_model_read(const char *path, irmv_number_model *m, float *buf, int64_t buf_floats, int64_t *need_floats)
{
    if (!path || !m) return fail(IRMV_ERR_ARG, "number_model_read: path / model is null");
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return fail(IRMV_ERR_MODEL, std::string("number_model_read: cannot open ") + path);
    const int64_t size = (int64_t)f.tellg();
    if (size < (int64_t)kNumFileHeader) return fail(IRMV_ERR_ARG, "number_model_read: the file is shorter than its header");
    f.seekg(0);
    char head[kNumFileHeader];
    if (!f.read(head, sizeof head)) return fail(IRMV_ERR_MODEL, "number_model_read: read failed");
    uint32_t version;
    int32_t n_layers, dims[4], input;
    memcpy(&version, head + 4, 4); memcpy(&n_layers, head + 8, 4); memcpy(dims, head + 12, 16); memcpy(&input, head + 28, 4);
    if (memcmp(head, "IRMN", 4) != 0 || version != 1u) return fail(IRMV_ERR_ARG, "number_model_read: not an .irmn file of version 1");
    TRY(check_number_shape(n_layers, dims, input, "number_model_read"));   // (bounds every length below)
    int64_t need = 0;
    for (int l = 0; l < n_layers; l++) need += (int64_t)dims[l] * dims[l + 1] + dims[l + 1];
    if (need > kNumFileFloatsMax || size != (int64_t)kNumFileHeader + need * 4) return fail(IRMV_ERR_ARG, "number_model_read: the file's size is not that of its header's model");
    if (need_floats) *need_floats = need;
    if (!buf || buf_floats < need) return fail(IRMV_ERR_ARG, "number_model_read: buf is too small");
    if (!f.read(reinterpret_cast<char *>(buf), need * 4)) return fail(IRMV_ERR_MODEL, "number_model_read: read failed");
    memset(m, 0, sizeof *m);
    m->struct_size = sizeof *m;
    m->n_layers = n_layers; m->input = input;
    for (int l = 0; l < 4; l++) m->dims[l] = dims[l];
    float *at = buf;
    for (int l = 0; l < n_layers; l++) {
        m->weight[l] = at; at += (size_t)dims[l] * dims[l + 1];
        m->bias[l] = at; at += dims[l + 1];
    }
    return IRMV_OK;
}

extern "C" int irmv_engine_load_number_model(irmv_engine *e, const char *path)
{
    std::vector<float> buf((size_t)kNumFileFloatsMax);
    irmv_number_model m;
    TRY(irmv_number_model_read(path, &m, buf.data(), (int64_t)buf.size(), nullptr));
    return irmv_engine_set_number_model(e, &m);
}

static int check_number_opts(const irmv_number_opts *o)
{
    if (!o) return fail(IRMV_ERR_ARG, "numbers: opts is null");
    if (o->struct_size != sizeof(irmv_number_opts)) return fail(IRMV_ERR_ARG, "numbers: opts.struct_size is not sizeof(irmv_number_opts)");
    if (o->enable != 0 && o->enable != 1) return fail(IRMV_ERR_ARG, "numbers: enable must be 0 or 1");
    if (o->reserved[0] != 0 || o->reserved[1] != 0 || o->reserved[2] != 0) return fail(IRMV_ERR_ARG, "numbers: reserved must be 0");
    return IRMV_OK;
}

// The first irmv_engine_set_numbers: the patches where they were never set, the records (device and pinned, zeroed), the op
// and the one re-capture.  Nothing of the engine is in flight.
static int enable_numbers(irmv_engine *e)
{
    bool dropped = false;
    if (e->patch_op < 0) {
        TRY(enable_patches(e));   // (drops the graphs)
        patch_opts_defaults(&e->patch_opts);
        e->patch_opts.enable = 1;
        TRY(write_patch_table(e));
        dropped = true;
    }
    const size_t n = (size_t)e->cfg.num_slots * e->cfg.max_det;
    // DevNumber: labels and logits that only the host reads; number_step_kernel writes every word of the records of [0, num_dets)
    // where it is enabled, no kernel reads one
    TRY(dev_alloc(e, (void **)&e->number.dev, n * sizeof(DevNumber), "number_dev", mem_scratch(MEM_U8)));
    TRY(e->number.pin(e, e->cfg.num_slots, e->cfg.max_det, "pinned number_host"));
    append_op(e, OP_NUMBER);
    if (!dropped) drop_graphs(e, false);   // (run_post's graphs too: the op stands behind their patch launch)
    return IRMV_OK;
}

extern "C" int irmv_engine_set_numbers(irmv_engine *e, const irmv_number_opts *o)
{
    TRY(check_number_opts(o));
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (o->enable && !e->number_model) return fail(IRMV_ERR_ARG, "numbers: enable needs a model (irmv_engine_set_number_model)");
    if (e->number_op < 0 && !o->enable) { e->number_opts = *o; return IRMV_OK; }   // never enabled: nothing to switch off, nothing is made
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    if (e->number_op < 0) TRY(enable_numbers(e));
    if (!o->enable) TRY(e->number.zero(e->cfg.num_slots));   // nothing writes the records from here on
    e->number_opts = *o;
    return write_number_table(e);
}

extern "C" int irmv_engine_get_numbers(const irmv_engine *e, irmv_number_opts *o)
{
    if (!e || !o) return fail(IRMV_ERR_ARG, "engine / opts is null");
    *o = e->number_opts;
    return IRMV_OK;
}

// A step's numbers: they read the patch records where the step's patch op wrote them and go where the step's records go
// (Records::step_at), as launch_patch reads the DevDet records of pa.
void irmv::launch_number(const irmv_engine *e, const Step &s, const PostArgs &pa, hipStream_t st)
{
    NumberArgs a{};
    a.patches = e->patch.step_at(e, s);
    a.max_det = e->cfg.max_det;
    a.num_dets = reinterpret_cast<const int *>(pa.fout);
    a.num_dets_stride = (int)(sizeof(DevFrameOut) / sizeof(int));
    a.table = e->number_table_dev;
    a.weights = e->number_weights;
    a.bias = e->number_bias;
    a.out = e->number.step_at(e, s);
    launch_number_step(a, s.count, st);
}

extern "C" int irmv_engine_plate_numbers(irmv_engine *e, int slot, irmv_plate_number *out, int cap, int *n)
{
    TRY(check_range(e, slot, 1));
    if (!n || (cap > 0 && !out)) return fail(IRMV_ERR_ARG, "out/n is null");
    if (e->number_op < 0) return fail(IRMV_ERR_ARG, "irmv_engine_plate_numbers: irmv_engine_set_numbers has not been called on this engine");
    return e->number.deliver(e, slot, out, cap, n);
}

extern "C" int irmv_engine_numbers_at(irmv_engine *e, const irmv_plate_patch *patches, int n, irmv_plate_number *out)
{
    if (n < 0 || n > kMaxDetCap || (n > 0 && (!patches || !out))) return fail(IRMV_ERR_ARG, "numbers_at: n must be 0..IRMV_MAX_DET_CAP with patches/out set");
    for (int i = 0; i < n; i++) {
        if (patches[i].state != 0 && patches[i].state != 1) return fail(IRMV_ERR_ARG, "numbers_at: a patch's state must be 0 or 1");
        if (patches[i].otsu < 0 || patches[i].otsu > 255) return fail(IRMV_ERR_ARG, "numbers_at: a patch's otsu must be 0 .. 255");
    }
    if (!e) return fail(IRMV_ERR_ARG, "engine is null");
    if (!e->number_model) return fail(IRMV_ERR_ARG, "numbers_at: the engine has no model (irmv_engine_set_number_model)");
    if (n == 0) return IRMV_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    TRY(irmv_engine_wait(e));
    hipStream_t st = e->stream;
    // the call's buffers: the host uploads the n patch records a call reads (bytes that are compared and converted, never an
    // index), the kernel writes every word of the n records the host copies out
    if (!e->number_at_in) TRY(dev_alloc(e, (void **)&e->number_at_in, (size_t)kMaxDetCap * sizeof(DevPatch), "number_at_in", mem_scratch(MEM_U8)));
    if (!e->number_at_out) TRY(dev_alloc(e, (void **)&e->number_at_out, (size_t)kMaxDetCap * sizeof(DevNumber), "number_at_out", mem_scratch(MEM_U8)));
    HIP_TRY(hipMemcpyAsync(e->number_at_in, patches, (size_t)n * sizeof(DevPatch), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (`patches` is the caller's pageable memory)
    NumberArgs a{};
    a.patches = e->number_at_in;
    a.max_det = e->cfg.max_det;
    a.table = e->number_table_dev;
    a.weights = e->number_weights;
    a.bias = e->number_bias;
    a.out = e->number_at_out;
    launch_number_points(a, n, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, e->number_at_out, (size_t)n * sizeof(DevNumber), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return IRMV_OK;
}

extern "C" int irmv_number_limits(int32_t out[8])
{
    if (!out) return fail(IRMV_ERR_ARG, "out is null");
    out[0] = kNumIn; out[1] = kNumHiddenMax; out[2] = kNumClassMax; out[3] = kNumLayersMax;
    out[4] = (int32_t)sizeof(irmv_plate_number); out[5] = kNumWeightHalves; out[6] = (int32_t)kNumValueMax; out[7] = 0;
    return IRMV_OK;
}

extern "C" int irmv_number_softmax(const irmv_plate_number *rec, int C, float out[16])
{
    if (!rec || !out || C < 1 || C > kNumClassMax) return fail(IRMV_ERR_ARG, "number_softmax: rec / out is null or C outside 1 .. 16");
    for (int i = 0; i < kNumClassMax; i++) out[i] = 0.0f;
    if (rec->state != 1) return IRMV_OK;
    double mx = rec->logits[0], sum = 0.0, ex[kNumClassMax];
    for (int i = 1; i < C; i++) mx = std::max(mx, (double)rec->logits[i]);
    for (int i = 0; i < C; i++) { ex[i] = std::exp((double)rec->logits[i] - mx); sum += ex[i]; }
    for (int i = 0; i < C; i++) out[i] = (float)(ex[i] / sum);
    return IRMV_OK;
}
