// Everything an engine decides by timing at its creation: each conv's tile (and the process-wide cache of those choices), the
// grouped Detect-branch launches, and the launch form of a synchronous single-frame step.
#include "engine_internal.hpp"

// tile choices already measured in this process, keyed by layer shape and batch (engines are created
// repeatedly in tests and by multi-slot nodes; the kernels and the device do not change in between)
// Process-wide and shared by every engine on every thread: all accesses hold g_tune_mu.
static bool operator==(const TuneEntry &x, const TuneEntry &y) { return x.mt == y.mt && x.nt == y.nt && x.flags == y.flags && x.ipw == y.ipw; }
static std::mutex g_tune_mu;
static std::map<std::string, TuneEntry> g_tune_cache;
static std::set<std::string> g_tune_files;   // IRMV_TUNE_CACHE paths already read

// A tile's family and options as one word (the cache file's third column): LDS family, deep prefetch, direct kernel in the
// LDS family's K order, pointwise kernel, two- / four-step staging, LDS family chunk-major over 2 / 4 images, 8-wave
// workgroup, resident weights (ipw = images per workgroup, any value), their ping-pong form
enum : int { T_LDS = 1, T_DEEP = 2, T_CT = 4, T_PW = 8, T_PF2 = 16, T_PF4 = 32, T_CM2 = 64, T_CM4 = 128, T_W8 = 256, T_WR = 512, T_PP = 1024 };
static int tile_flags(const ConvCfg &c)
{
    return (c.lds ? T_LDS : 0) | (c.deep ? T_DEEP : 0) | (c.ct ? T_CT : 0) | (c.pw ? T_PW : 0) | (c.pf2 ? T_PF2 : 0) | (c.pf4 ? T_PF4 : 0) |
           (c.cm == 2 ? T_CM2 : 0) | (c.cm == 4 ? T_CM4 : 0) | (c.w8 ? T_W8 : 0) | (c.wr ? T_WR : 0) | (c.pp ? T_PP : 0);
}
TuneEntry irmv::tune_entry(const ConvCfg &c) { return {c.mt, c.nt, tile_flags(c), c.ipw}; }

// IRMV_TUNE_CACHE=<file>: persist the measured choices so that a profiled run (rocprofv3 --pmc ...)
// replays exactly the tiles of the benchmarked run without the tuning launches in its trace.  A path is read the first
// time an engine sees it; its entries replace the process's own for the same key.
static void tune_cache_load()
{
    const char *path = getenv("IRMV_TUNE_CACHE");
    if (!path) return;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (!g_tune_files.insert(path).second) return;
    std::ifstream f(path);
    std::string key;
    TuneEntry t;
    while (f >> key >> t.mt >> t.nt >> t.flags >> t.ipw) g_tune_cache[key] = t;
}

static void tune_cache_save()
{
    const char *path = getenv("IRMV_TUNE_CACHE");
    if (!path) return;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    std::ofstream f(path);
    for (auto &kv : g_tune_cache) f << kv.first << ' ' << kv.second.mt << ' ' << kv.second.nt << ' ' << kv.second.flags << ' ' << kv.second.ipw << '\n';
}

// ---- per-layer tile autotuner ---------------------------------------------------
// Every conv layer is timed at its real shape with each (MT, NT) tile the kernel
// family offers and keeps the fastest, once for full batched steps and once for
// single-frame steps.  All tiles walk K in the same order, so the choice never
// changes a single output bit (tests/test_gpu_engine.py::test_tile_choice_is_bitwise_neutral).

// A candidate of the autotuner: the layer's own configuration with a tile shape, family and options (tile_flags' word).
static ConvCfg tile_cfg(const ConvCfg &base, int mt, int nt, int flags, int ipw)
{
    ConvCfg c = base;
    c.mt = mt; c.nt = nt; c.ipw = ipw;
    c.lds = flags & T_LDS; c.deep = flags & T_DEEP; c.ct = flags & T_CT; c.pw = flags & T_PW; c.pf2 = flags & T_PF2; c.pf4 = flags & T_PF4;
    c.cm = (flags & T_CM2) ? 2 : ((flags & T_CM4) ? 4 : 0); c.w8 = flags & T_W8; c.wr = flags & T_WR; c.pp = flags & T_PP;
    return c;
}

// Every candidate of one conv layer at one batch, in the order the tuner times them (IRMV_AUTOTUNE=0 takes the first that
// runs; a cached choice is replayed only if it is one of them).  Launches nothing: a candidate is listed if resolve_conv
// finds a kernel for it on this layer, the one that run_conv launches.  lds_ok: the layer's kernel family; want_fuse: the
// fused 1x1 epilogue, which needs an LDS-family tile that owns all 64 channels (nt = 4).
std::vector<TuneCand> irmv::tune_candidates(const Op &op, const ConvArgs &a, int count, bool want_fuse, bool lds_ok, const TuneSwitches &sw, int num_cus)
{
    std::vector<TuneCand> v;
    // IRMV_FORCE_S2=lds|ct|deep (parity test): the stride-2 layers of the LDS family on ONE of their three bit-identical
    // implementations -- the LDS kernel, the direct kernel walking K chunk-major, its deep-prefetch form
    const bool s2 = sw.has_s2 && lds_ok && op.cfg.stride == 2;
    const ConvWeights w = conv_weights(op);
    auto add = [&](const ConvCfg &c, bool forced = false) {
        if (s2 && !forced && sw.force_s2 != (c.lds ? "lds" : (c.deep ? "deep" : "ct"))) return;
        if (resolve_conv(c, a, w, count)) v.push_back({c, forced});
    };
    const int ipw_max = lds_ok ? std::min(4, count) : 1;
    for (int mt = 1; mt <= 4; mt *= 2)
        for (int nt = 1; nt <= 4; nt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
                if (!want_fuse || nt == 4) add(tile_cfg(op.cfg, mt, nt, lds_ok ? T_LDS : 0, ipw));
    // LDS family, smallest pixel tile, staging two steps ahead (layers whose step is shorter than a memory round trip)
    if (lds_ok && !want_fuse && !sw.no_pf2)
        for (int nt = 1; nt <= 4; nt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2) add(tile_cfg(op.cfg, 1, nt, T_LDS | T_PF2, ipw));
    // ... and four steps ahead: layers of four or more chunks on maps small enough for four register sets (a lone frame's
    // 20 x 20 layers: every step of a workgroup in flight at once)
    if (lds_ok && !want_fuse && !sw.no_pf4 && op.cin >= 128) add(tile_cfg(op.cfg, 1, 1, T_LDS | T_PF4, 1), sw.force_pf4);
    // LDS family, chunk-major over the workgroup's images: a chunk's weights staged once for all of them
    if (lds_ok && !sw.no_cm)
        for (int mt = 1; mt <= 2; mt *= 2)
            for (int ipw = 2; ipw <= std::min(mt == 1 ? 4 : 2, count); ipw *= 2)
                add(tile_cfg(op.cfg, mt, 4, T_LDS | (ipw == 2 ? T_CM2 : T_CM4), ipw), sw.force_cm);
    // LDS family, stride 2: one 8-wave workgroup per CU on a block twice as tall (mt = 2 fits LDS, weights staged for
    // twice the pixels)
    if (lds_ok && op.cfg.stride == 2 && !want_fuse && !sw.no_w8)
        for (int mt = 1; mt <= 2; mt *= 2)
            for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
                for (int cmv = 0; cmv < 2; cmv++)
                    add(tile_cfg(op.cfg, mt, 4, T_LDS | T_W8 | (cmv ? (ipw == 2 ? T_CM2 : T_CM4) : 0), ipw), sw.force_w8);
    // ... and with all of 128 output channels per workgroup (nt = 8, mt = 1): these layers are bound by what a CU can stage
    // from L2 (12 B/clk), and the stride-2 patch -- four input pixels per output pixel -- is then fetched once per 128
    // channels instead of once per 64; chunk-major over two images halves the weight staging on top
    if (lds_ok && op.cfg.stride == 2 && !want_fuse && !sw.no_w8 && !sw.no_nt8)
        for (int ipw = 1; ipw <= ipw_max; ipw *= 2)
            for (int cmv = 0; cmv < 2; cmv++)
                add(tile_cfg(op.cfg, 1, 8, T_LDS | T_W8 | (cmv ? T_CM2 : 0), ipw), sw.force_nt8);
    // LDS family, Cin = Cout = 64, stride 1: resident weights (one 8-wave workgroup per CU walks ipw images at its tile
    // position; lockstep, or as two ping-pong groups of four waves).  ipw: the smallest that lets the chip hold the
    // grid in one round, and half of it.
    if (lds_ok && count >= 2 && !sw.no_wres)
        for (int ppv = 0; ppv < 2; ppv++) {
            const int wgt = conv_wres_tiles(a, op.cfg.stride, ppv != 0);
            if (wgt <= 0) continue;
            int ipw1 = 1;
            while (ipw1 < count && (long)wgt * ((count + ipw1 - 1) / ipw1) > num_cus) ipw1++;
            const int cand[3] = {ipw1, (ipw1 + 1) / 2, std::min(count, 2 * ipw1)};
            for (int k = 0; k < 3; k++)
                if (k == 0 || (cand[k] != cand[0] && (k == 1 || cand[2] != cand[1]))) add(tile_cfg(op.cfg, 2, 4, T_LDS | T_WR | (ppv ? T_PP : 0), cand[k]));
        }
    // parity tests: IRMV_FORCE_WRES=<n> puts every eligible layer on the resident-weights kernel with n images per
    // workgroup -- the ping-pong form (listed last, so it wins) where the map tiles into its blocks (n < 0: never), else the
    // lockstep form
    if (sw.has_wres && lds_ok && count >= 2) {
        const int n = atoi(sw.force_wres.c_str());
        for (int ppv = 0; ppv <= (n > 0 ? 1 : 0); ppv++) add(tile_cfg(op.cfg, 2, 4, T_LDS | T_WR | (ppv ? T_PP : 0), std::max(1, std::min(count, n < 0 ? -n : n))), true);
    }
    // 1x1 layers: the persistent pointwise kernel (same operands, same k order as the direct kernel)
    if (conv_pw_eligible(op.cfg, a) && !sw.no_pw) {
        add(tile_cfg(op.cfg, 2, 4, T_PW, 1), sw.force_pw);
        // ... and its multi-block form: one workgroup runs a pixel tile against 2 / 4 output-channel blocks (input read once)
        for (int nbw = 2; nbw <= 4 && !sw.no_pwn; nbw *= 2)
            add(tile_cfg(op.cfg, 2, 4, T_PW, nbw), sw.force_pwn);   // (forced: the widest form offered)
    }
    // A layer of the LDS family may also run on the direct kernel walking K in that family's order on its weights (ct):
    // bit-identical, so the family rule still holds.  Offered where the direct kernel has a chance: stride 2.
    if (lds_ok && !want_fuse && op.cfg.stride == 2 && !op.cfg.cin16)
        for (int mt = 1; mt <= 4; mt *= 2)
            for (int nt = 1; nt <= 4; nt *= 2) add(tile_cfg(op.cfg, mt, nt, T_CT, 1));
    // single-frame steps: the latency variants of the direct kernel (deep prefetch ring), same rule.
    // Batched steps: offered to the 1x1 layers only (4..16 k-steps: the ring then holds the wave's whole K range).
    if ((count == 1 || op.cfg.ks == 1) && !want_fuse && !sw.no_deep && !op.cfg.cin16 && !op.cfg.out_f32 && op.cfg.act == 1) {
        const int tiles[4][2] = {{1, 1}, {2, 1}, {1, 2}, {1, 4}};
        for (auto &t : tiles) add(tile_cfg(op.cfg, t[0], t[1], T_DEEP | (lds_ok ? T_CT : 0), 1));
    }
    return v;
}

ConvView irmv::conv_view(const irmv_engine *e, const Op &op, int first, int count)
{
    ConvView v;
    const ConvWeights w = conv_weights(op);
    const bool fuse_k16 = op.fuse_next >= 0 && op.cfg.cin16;   // the keypoint final in the direct kernel's epilogue: any pixel tile (nt = 1 is the layer's only one)
    v.want_fuse = op.fuse_next >= 0 && !fuse_k16;
    fill_conv_args(e, op, first, count, v.a, v.want_fuse || fuse_k16);
    if (v.want_fuse) {   // the fused epilogue needs an LDS-family tile that owns all 64 channels (nt = 4)
        bool f_ok = false;
        for (int mt = 1; mt <= 4 && !f_ok; mt *= 2) f_ok = conv_lds_fits(v.a, w, op.cfg.stride, mt, 4);
        if (!f_ok) {
            v.want_fuse = false;
            fill_conv_args(e, op, first, count, v.a, false);
        }
    }
    // Kernel family by a rule that does not depend on the batch (the two families walk K in
    // different orders): LDS-staged whenever some tile of it fits this layer, else direct.
    v.lds_ok = false;
    if (op.cfg.ks == 3 && op.cfg.act == 1 && !op.cfg.out_f32)
        for (int mt = 1; mt <= 4 && !v.lds_ok; mt *= 2)
            for (int nt = 1; nt <= 4 && !v.lds_ok; nt *= 2) v.lds_ok = conv_lds_fits(v.a, w, op.cfg.stride, mt, nt);
    return v;
}

int irmv::autotune_convs(irmv_engine *e)
{
    const TuneSwitches &sw = e->sw.tune;
    tune_cache_load();
    hipEvent_t ea, eb;
    HIP_TRY(hipEventCreate(&ea));
    HIP_TRY(hipEventCreate(&eb));
    const int counts[2] = {stream_share(e, e->cfg.num_slots), 1};   // the batch one graph actually runs; single frame
    for (Op &op : e->ops) {
        if (op.kind != OP_CONV) continue;
        for (int pass = 0; pass < (counts[0] > 1 ? 2 : 1); pass++) {
            const int count = counts[pass];
            op.tune_fuse[pass] = op.fuse_next;
            const ConvView v = conv_view(e, op, 0, count);
            if (!v.want_fuse && !op.cfg.cin16) op.fuse_next = -1;   // no tile can carry the 1x1: the layers stay apart
            const ConvArgs &a = v.a;
            const bool want_fuse = v.want_fuse, lds_ok = v.lds_ok;
            char key[160];
            snprintf(key, sizeof key, "gfx950.t5|%d.%d.%d.%d.%d.%d|%dx%d>%dx%d|c%d.%d.%d.%d>%d|ld%d.%d.%d|n%d|%d", op.cfg.ks, op.cfg.stride,   // ".t5": the table format / flag set of round 5 -- entries of another round's file never match, so they are re-tuned, not reinterpreted
                     (int)op.cfg.cin16, op.cfg.act, (int)op.cfg.out_f32, (int)lds_ok, a.Hin, a.Win, a.Hout, a.Wout, a.s0.C, a.s1.C, a.s0.shift,
                     a.s1.shift, a.cout_pad, a.s0.ld, a.s1.ld, a.out_ld, count, (a.res ? 1 : 0) + 2 * a.n2);
            const std::vector<TuneCand> cands = tune_candidates(op, a, count, want_fuse, lds_ok, sw, e->num_cus);
            // a forced layer neither replays a cached choice nor leaves its own for a later engine; nor does an untuned one
            const bool forced = (sw.has_s2 && lds_ok && op.cfg.stride == 2) || std::any_of(cands.begin(), cands.end(), [](const TuneCand &k) { return k.forced; });
            ConvCfg best_cfg = pass == 0 ? op.cfg : op.cfg_one;
            bool have_hit = false;
            if (!forced && !sw.untuned && !sw.verbose) {   // a cached choice (this process, or an IRMV_TUNE_CACHE file) is replayed if it is a candidate
                std::lock_guard<std::mutex> lk(g_tune_mu);
                auto hit = g_tune_cache.find(key);
                if (hit != g_tune_cache.end()) {
                    const TuneEntry &h = hit->second;
                    auto it = std::find_if(cands.begin(), cands.end(), [&](const TuneCand &k) { return tune_entry(k.c) == h; });
                    if (it != cands.end()) { best_cfg = it->c; have_hit = true; }
                    else if (sw.warn) fprintf(stderr, "[autotune] cached tile for %s rejected (mt %d nt %d lds %d ipw %d): re-tuning\n", key, h.mt, h.nt, h.flags & 1, h.ipw);
                }
            }
            float best = 1e30f;
            for (size_t i = 0; i < cands.size() && !have_hit; i++) {
                const ConvCfg &c = cands[i].c;
                if (cands[i].forced) {
                    if (run_conv(op, c, a, count, e->stream)) { best = 0.f; best_cfg = c; }
                    continue;
                }
                if (sw.untuned && best < 1e29f) continue;   // IRMV_AUTOTUNE=0: the first candidate that runs is the choice
                bool ok = true;
                for (int r = 0; r < 2 && ok; r++) ok = run_conv(op, c, a, count, e->stream);
                if (!ok) continue;
                if (sw.untuned) { best = 0.f; best_cfg = c; continue; }
                float ms = 1e30f;   // best of 3 bursts of 4
                for (int rep = 0; rep < 3; rep++) {
                    HIP_TRY(hipEventRecord(ea, e->stream));
                    for (int r = 0; r < 4; r++) run_conv(op, c, a, count, e->stream);
                    HIP_TRY(hipEventRecord(eb, e->stream));
                    HIP_TRY(hipEventSynchronize(eb));
                    float t = 0.f;
                    HIP_TRY(hipEventElapsedTime(&t, ea, eb));
                    ms = t < ms ? t : ms;
                }
                if (sw.verbose) {
                    char nm[48];
                    conv_cfg_name(c, nm, sizeof nm);
                    fprintf(stderr, "[autotune] %-22s count=%-2d %-28s %8.2f us\n", op.layer.c_str(), count, nm, ms / 4 * 1e3);
                }
                if (ms < best) { best = ms; best_cfg = c; }
            }
            if (!forced && !sw.untuned) { std::lock_guard<std::mutex> lk(g_tune_mu); g_tune_cache[key] = tune_entry(best_cfg); }
            if (pass == 0) { op.cfg = best_cfg; conv_cfg_name(op.cfg, op.kname, sizeof op.kname); }
            else { op.cfg_one = best_cfg; conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one); }
            if (counts[0] == 1) { op.cfg_one = op.cfg; conv_cfg_name(op.cfg_one, op.kname_one, sizeof op.kname_one); }
        }
    }
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    HIP_TRY(hipGetLastError());
    tune_cache_save();
    return IRMV_OK;
}

// ---- grouped Detect-branch launches (single-frame engines) ---------------------------
int irmv::build_head_groups(irmv_engine *e)
{
    if (!e->merge_head0 || !e->sw.group_head) return IRMV_OK;
    auto find_op = [&](const std::string &layer) {
        for (size_t i = 0; i < e->ops.size(); i++)
            if (e->ops[i].kind == OP_CONV && !e->ops[i].fused_away && e->ops[i].layer == layer) return (int)i;
        return -1;
    };
    auto time_of = [&](auto &&launch) {   // ms per launch, or < 0 if it cannot run
        for (int i = 0; i < 2; i++) if (!launch()) return -1.f;
        if (hipStreamSynchronize(e->stream) != hipSuccess) return -1.f;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1.f;
        (void)hipEventRecord(a, e->stream);
        for (int i = 0; i < 8; i++) launch();
        (void)hipEventRecord(b, e->stream);
        (void)hipEventSynchronize(b);
        float ms = -1.f;
        (void)hipEventElapsedTime(&ms, a, b);
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        return ms / 8.f;
    };
    auto members_time = [&](const std::vector<int> &mem) {
        return time_of([&] {
            for (int i : mem) {
                const Op &op = e->ops[i];
                ConvArgs a;
                fill_conv_args(e, op, 0, 1, a, true);
                if (!run_conv(op, op.cfg_one, a, 1, e->stream)) return false;
            }
            return true;
        });
    };
    auto try_group = [&](std::vector<int> mem, int family, std::vector<int> nts, const char *label) {
        for (int i : mem) if (i < 0) return;
        if (mem.size() < 2 || mem.size() > (size_t)kMultiMax) return;
        irmv_engine::HeadGroup best;
        float best_ms = -1.f;
        for (int nt : nts) {
            irmv_engine::HeadGroup g;
            g.members = mem; g.family = family; g.nt = nt;
            if (family == 1) {
                g.cfg = e->ops[mem[0]].cfg_one;
                bool same = !g.cfg.lds && !g.cfg.ct && !g.cfg.pw;   // (the members' own tile shapes and prefetch depths are bitwise neutral: the group runs mt = nt = 1)
                for (int i : mem) {
                    const ConvCfg &c = e->ops[i].cfg_one;
                    same = same && c.ks == g.cfg.ks && c.stride == g.cfg.stride && c.cin16 == g.cfg.cin16 && c.act == g.cfg.act && c.out_f32 == g.cfg.out_f32 && !c.lds && !c.ct && !c.pw;
                }
                if (!same) continue;
                g.cfg.mt = g.cfg.nt = 1; g.cfg.deep = false;
            } else {
                bool fam = true;   // every member must belong to the LDS family's K order (its single-frame choice is an LDS tile or the CT stand-in)
                for (int i : mem) fam = fam && (e->ops[i].cfg_one.lds || e->ops[i].cfg_one.ct);
                if (!fam) continue;
            }
            if (e->sw.group_verbose) { fprintf(stderr, "[irmv group] timing %s nt %d ...\n", label, nt); fflush(stderr); }
            const float ms = time_of([&] { return launch_head_group(e, g, 0, nullptr, 0u, e->stream); });
            if (e->sw.group_verbose) { fprintf(stderr, "[irmv group] ... %.2f us\n", ms * 1e3f); fflush(stderr); }
            if (ms > 0.f && (best_ms < 0.f || ms < best_ms)) { best_ms = ms; best = g; }
        }
        if (best_ms < 0.f) return;
        const float sep = members_time(mem);
        if (e->sw.tune.verbose || e->sw.group_verbose) fprintf(stderr, "[irmv group] %s: %zu convs, one launch %.2f us, separate %.2f us\n", label, mem.size(), best_ms * 1e3f, sep * 1e3f);
        if (sep > 0.f && best_ms >= sep && !e->sw.group_force) return;   // IRMV_GROUP_FORCE=1 (parity test): group even where the one launch timed slower
        if (family == 0) snprintf(best.name, sizeof best.name, "%s_lds_mt1_nt%d_x%zu", label, best.nt, mem.size());
        else snprintf(best.name, sizeof best.name, "%s_direct_x%zu", label, mem.size());
        const int gi = (int)e->head_groups.size();
        e->head_groups.push_back(best);
        for (int i : mem) e->ops[i].group = gi;
    };
    const bool kpt = e->nk > 0;
    std::vector<int> g1, g2, g3, g4;
    bool g2_fused = true;
    for (int i = 0; i < 3; i++) {
        const std::string si = std::to_string(i);
        g1.push_back(find_op("model.22.s0." + si));
        const int c2 = find_op("model.22.cv2." + si + ".1"), c3 = find_op("model.22.cv3." + si + ".1");
        g2.push_back(c2); g2.push_back(c3);
        g2_fused = g2_fused && c2 >= 0 && c3 >= 0 && e->ops[c2].fuse_next >= 0 && e->ops[c3].fuse_next >= 0;
        if (kpt) { g3.push_back(find_op("model.22.cv4." + si + ".1")); g4.push_back(find_op("model.22.cv4." + si + ".2")); }
    }
    try_group(g1, 0, {1, 2}, "head_s0");
    if (g2_fused) try_group(g2, 0, {4}, "head_s1+1x1");
    // A group is launched where its FIRST member stands in the op list, so every member's input must exist by then.  The
    // first-stage convs precede all of these; the keypoint finals (cv4.i.2) read cv4.i.1, and cv4.1.1 / cv4.2.1 stand BEHIND
    // cv4.0.2 in the list: the finals may only be grouped when the convs before them are (one launch, at cv4.0.1's place).
    if (kpt) {
        const size_t before = e->head_groups.size();
        try_group(g3, 1, {1}, "head_kpt1");
        bool k16 = false;   // (finals on the 16x16x16 MFMA are fused into the convs in front of them, or run their own kernel: the grouped direct kernel would give other bits)
        for (int i : g4) k16 = k16 || i < 0 || e->ops[i].w_k16 != nullptr;
        if (e->head_groups.size() > before && !k16) try_group(g4, 1, {1}, "head_kpt2");
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return IRMV_OK;
}

// Which launch form serves detect() on this box: both timed on slot 0 (whatever its pinned slot holds: zeros at creation), the
// eager one kept only if it is at least 1 % faster.  IRMV_SYNC_LAUNCH=graph|eager skips the timing.
int irmv::choose_sync_launch(irmv_engine *e)
{
    if (e->sw.sync_launch >= 0) { e->sync_launch = e->sw.sync_launch; return IRMV_OK; }
    double t[2] = {0.0, 0.0};
    for (int round = 0; round < 2; round++)
        for (int mode = 0; mode < 2; mode++) {
            e->sync_launch = mode;
            for (int i = 0; i < 24; i++) {
                const auto t0 = std::chrono::high_resolution_clock::now();
                TRY(irmv_engine_submit(e, 0, 1, IRMV_SUBMIT_H2D));
                TRY(irmv_engine_wait_slots(e, 0, 1));
                if (i >= 8) t[mode] += std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count();
            }
        }
    e->sync_launch = t[1] < 0.99 * t[0] ? 1 : 0;
    if (e->sw.tune.verbose) fprintf(stderr, "[irmv] synchronous single-frame step: graph replay %.1f us, eager launches %.1f us -> %s\n", t[0] / 32, t[1] / 32, e->sync_launch ? "eager" : "graph");
    return IRMV_OK;
}
