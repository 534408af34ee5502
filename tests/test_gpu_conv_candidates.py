"""Every conv layer on its own, every autotuner candidate included, against a per-layer fp64 reference.

The conv autotuner (engine_tune.cpp autotune_convs) times every candidate tune_candidates() lists for a layer and keeps the
fastest, on the claim that all of them compute the same bits.  Here every candidate of every conv op is run through the
C ABI's test hooks (irmv_engine_conv_candidates / irmv_engine_run_conv_candidate) on every slot range production can run
it on: the tune count itself, the other stream shares (first > 0, the remainder share), a partial count, and for the
single-frame choice the last slot.  Before each run the hook fills the output channels the run must write, on its slots,
with NaN (for a Detect carrier: the head slice its fused 1x1 writes).  After it the op's output tensor(s) must be bitwise
as the engine's real step left them: every value rewritten, bitwise the engine's own choice and the step, nothing outside
[first, first + count) or outside the op's channels touched.  (Each op also shows once that the NaN fill alone fails
the comparison.)  Engines of more than 8 slots compare a sample: the first and last slot of every range, their
neighbours, and both sides of the first and last ipw boundary in it -- where a dropped partial workgroup would show.

The engine's result for each layer is then compared with tests/conv_ref.py (float64) on that slot's own input tensors,
per element, under the bound

    |y_gpu - y_ref| <= 2^-11 |y_ref| (1 + M_REL) + C_ACC 2^-24 (|b| + sum |w| |x|) + 2^-24 ln 2

  * 2^-11 |y_ref|: the engine stores s = fp16(log2(e) y) (irmv_common.hpp, "activation scale"): one rounding to fp16.
    M_REL covers that the value rounded is itself off by the terms below and the read-back's fp32 multiply by ln 2.
  * C_ACC 2^-24 (|b| + sum |w||x|): float32 accumulation in the MFMA K loop, the fp32 bias, the exp2 / rcp SiLU
    approximations, the residual add -- all scaled by the layer's own sum of |w x|, not by a global constant.
  * 2^-24 ln 2: the fp16 subnormal step at the activation scale.
  * fp32 outputs (the Detect finals) drop the first and last terms.  A carrier's fused 1x1 adds sum |w2| * (the bound of
    its fp16 input) to its own accumulation term.

M_REL and C_ACC were set from the measured distribution (the worst err / bound per layer is printed to the test log for
every engine).  On every engine here the worst layer sits at 0.797 - 0.799 = 1 / (1 + M_REL): the largest error of
any layer is the half-ulp rounding of its fp16 store itself.  The fp32 Detect finals have no fp16 store, so only the
accumulation term bounds them, and there it is a handful of fp32 roundings that can each reach 2^-24 (|b| + sum |w||x|)
when the output barely cancels: the MFMA sum, the ln 2 unscale of the accumulator, the bias add, and the reference's
own fp32 read-back of its fp16 inputs.  The keypoint final model.22.cv4.0.2 (K = 16: one MFMA step, few terms, little
cancellation) comes closest: 0.876 on the 1024 engine, i.e. C_ACC ~ 3.5 -- four such roundings is what C_ACC = 4
allows.  (On written inputs of a wide range these finals pass 4: the MFMA rounds more often than once.  The count is in
tests/test_gpu_act_craft.py, "Finding".)  M_REL = 0.25 leaves a quarter of an fp16 step for the read-back and the pre-rounding error.  Both are far
below the ~K / 32 accumulator roundings a K loop makes at worst (144 for model.9.cv2).  A mis-staged chunk or a wrong
border tap moves outputs by a sizable fraction of sum |w||x| and lands far outside this bound; so does a bias error
wherever it is large against 2^-11 |y| (an error of one fp16 step of the bias passes where |y| >> |b|).  The end to
end bounds of tests/test_gpu_engine.py (EMU_TOL = 6e-2 on the taps, HEAD_TOL = 4e-2 on the head) accept such an
engine: test_per_layer_check_sees_what_the_end_to_end_bounds_miss below.

The 256-slot and 2048-net engines are the slow cases (test_slow_...; leave them out with -k "not slow").
"""
import ctypes as C
import time

import numpy as np
import pytest

import conv_ref
from irmv_detection_amd import arch, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle

pytestmark = pytest.mark.gpu

M_REL = 0.25
C_ACC = 4.0
U16, U32, FLOOR = 2.0 ** -11, 2.0 ** -24, 2.0 ** -24 * 0.693147180559945309
HEAD_TOL, EMU_TOL = 4e-2, 6e-2     # tests/test_gpu_engine.py


# ---- the hooks --------------------------------------------------------------------------------------------------
def conv_ops(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_conv_ops(e._h, None, 0, C.byref(n)))
    arr = (capi.ConvOp * n.value)()
    capi.check(e._L.irmv_engine_conv_ops(e._h, arr, n.value, C.byref(n)))
    return list(arr)


def candidates(e, op, tune_count):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_conv_candidates(e._h, op, tune_count, None, 0, C.byref(n)))
    arr = (capi.ConvCand * n.value)()
    capi.check(e._L.irmv_engine_conv_candidates(e._h, op, tune_count, arr, n.value, C.byref(n)))
    return list(arr)


def run(e, op, tune_count, cand, first, count, flags=capi.RUN_POISON):
    """Every run first fills the output it must write with NaN (capi.RUN_POISON): one that leaves a slot, a pixel tile or
    a channel unwritten cannot match what the step wrote."""
    return capi.check(e._L.irmv_engine_run_conv_candidate(e._h, op, tune_count, cand, first, count, flags), allow=(capi.DECLINED,))


def read(e, name, first, count):
    """Raw storage of slots [first, first + count): uint16 (fp16 bits) or float32, [count, H, W, C]."""
    shapes = e.__dict__.setdefault("_tensor_shapes", {})
    if name not in shapes:
        shape = (C.c_int * 3)()
        capi.check(e._L.irmv_engine_read_tap(e._h, 0, name.encode(), None, shape))   # every tensor an op names is a tap
        shapes[name] = tuple(shape)
    H, W, Cc = shapes[name]
    out = np.empty((count, H, W, Cc), np.float32 if name.startswith("head.") else np.uint16)
    capi.check(e._L.irmv_engine_read_tensor(e._h, name.encode(), first, count, out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def layer_table(blob):
    """weight layer name -> (w fp16 OHWI, b fp32) as the engine computes with, including the merged first-stage Detect
    convs of single-frame engines (engine_graph.cpp: cv2 / cv3 / cv4 .0 concatenated along cout, cv4 padded to 32 channels)."""
    hdr, layers = weights.parse_blob(blob)
    t = {sp.name: (w, b) for sp, w, b in layers}
    for i in range(3):
        br = ["cv2", "cv3"] + (["cv4"] if hdr["nk"] else [])
        cm = 160 if hdr["nk"] else 128
        w0 = t[f"model.22.cv2.{i}.0"][0]
        w = np.zeros((cm,) + w0.shape[1:], np.float16)
        b = np.zeros(cm, np.float32)
        for k, name in enumerate(br):
            wk, bk = t[f"model.22.{name}.{i}.0"]
            w[64 * k:64 * k + len(wk)], b[64 * k:64 * k + len(bk)] = wk, bk
        t[f"model.22.s0.{i}"] = (w, b)
    return t


# ---- the per-layer bound ------------------------------------------------------------------------------------------
def bound(y_ref, acc, f32):
    if f32:
        return C_ACC * U32 * acc
    return U16 * (1.0 + M_REL) * np.abs(y_ref) + C_ACC * U32 * acc + FLOOR


def layer_ratio(e, op, table, slot, cache):
    """max err / bound of the engine's output of op on one slot (and of its fused 1x1, if the step runs one)."""
    def tensor(name):
        if (name, slot) not in cache:
            cache[(name, slot)] = conv_ref.decode(read(e, name, slot, 1)[0], name)
        return cache[(name, slot)]
    names = {op.s0.tensor.decode(), op.s1.tensor.decode(), op.res.tensor.decode()} - {""}
    w, b = table[op.layer.decode()]
    fuse = table[op.fuse_layer.decode()] if op.fused else None
    r = conv_ref.op_forward(op, {n: tensor(n) for n in names}, w, b, fuse)
    y_ref, acc = r[0], r[1]
    out = tensor(op.out_tensor.decode())[..., op.out_coff:op.out_coff + op.cout]
    bd = bound(y_ref, acc, op.out_f32)
    ratio = float((np.abs(out - y_ref) / bd).max())
    if op.fused:
        y2, acc2 = r[2], r[3]
        w2 = np.abs(fuse[0].astype(np.float64))
        prop = conv_ref.conv(bd, w2, np.zeros(len(w2)), 1, 0)[0]          # sum |w2| * bound of the fp16 input
        head = tensor(op.fuse_tensor.decode())[..., op.fuse_coff:op.fuse_coff + op.fuse_cout]
        ratio = max(ratio, float((np.abs(head - y2) / (C_ACC * U32 * acc2 + prop)).max()))
    return ratio


def own_values(e, op, ops, share, cache):
    """Before op is checked: where other ops write the same channels of its output tensor (the bottleneck scratch of a
    C2f block with n > 1), that tensor holds the last writer's values -- rerun op's own choice on every slot.  Drop the
    cached read-backs of what op writes either way."""
    N = e.num_slots
    if any(o.op != op.op and o.out_tensor == op.out_tensor and o.out_coff < op.out_coff + op.cout_pad and
           op.out_coff < o.out_coff + o.cout_pad for o in ops):
        for f in range(0, N, share):
            assert run(e, op.op, share, -1, f, min(share, N - f)) == capi.OK
    for n in (op.out_tensor.decode(), op.fuse_tensor.decode()):
        for s in range(N):
            cache.pop((n, s), None)


# ---- the sweep ------------------------------------------------------------------------------------------------------
def ranges_for(tune_count, share, N):
    """Every kind of slot range production runs a tile tuned at tune_count on."""
    if tune_count == 1:
        r = [(0, 1), (N - 1, 1)]
    else:
        r = [(0, tune_count)] + [(f, min(share, N - f)) for f in range(share, N, share)] + [(1, tune_count - 1)]
    return list(dict.fromkeys(r))


def sampled_slots(N, share, ipws):
    """N <= 8: every slot.  Else the first and last slot of every range ranges_for() runs, the slots on both sides of
    them, and both sides of the first and last ipw boundary inside each range."""
    if N <= 8:
        return list(range(N))
    s = set()
    for f, c in ranges_for(share, share, N) + ranges_for(1, share, N):
        s.update((f - 1, f, f + c - 1, f + c))
        for p in ipws:
            if p < c:
                s.update((f + p - 1, f + p, f + (c - 1) // p * p - 1, f + (c - 1) // p * p))
    return sorted(v for v in s if 0 <= v < N)


def load_frames(e, N, seed0=0):
    for s in range(N):
        e.get_src_image_buffer(s)[:] = frames.synthetic_frame(seed0 + s)


def sweep(e, blob, log, ref_slots=None):
    """The whole per-layer check on engine e (frames loaded, nothing in flight).  Returns (checked, declined, total,
    per-layer worst ratio, failures)."""
    N = e.num_slots
    share = -(-N // e.num_streams)
    counts = [share, 1] if share > 1 else [1]
    e.submit(0, N)
    e.wait()
    ops = conv_ops(e)
    assert len(ops) >= 40
    for op in ops:
        assert op.fused == op.tune_fused, op.layer     # the step runs the epilogue the candidates were listed for
    heads0 = [e.read_head(s) for s in range(N)]
    raws0 = [e.read_raw(s) for s in range(N)]
    # what the step wrote, before anything else runs
    outs = sorted({op.out_tensor.decode() for op in ops} | {op.fuse_tensor.decode() for op in ops if op.fused})
    lazy = sorted({op.out_tensor.decode() for op in ops if op.out_lazy})
    step = {n: read(e, n, 0, N) for n in outs if n not in lazy}
    # tensors the step keeps on chip: recompute them on every slot (a read-back does), then nothing the step wrote moves
    if lazy:
        for s in range(N):
            e.read_tap(lazy[0], s)
    for n, v in step.items():
        assert np.array_equal(read(e, n, 0, N), v), f"materializing the fused layers changed {n}"
    table = layer_table(blob)
    check_slots = sampled_slots(N, share, ipws_all(e, ops, counts))
    def state(names):
        return {n: [read(e, n, s, 1) for s in check_slots] if N > 8 else read(e, n, 0, N) for n in names}
    def same(a, b):
        return all(np.array_equal(np.asarray(a[n]), np.asarray(b[n])) for n in a)
    checked = declined = total = 0
    failures, worst = [], {}
    cache = {}
    for op in ops:     # in step order: every op reads what the ops before it wrote
        names = [op.out_tensor.decode()] + ([op.fuse_tensor.decode()] if op.tune_fused else [])
        own_values(e, op, ops, share, cache)
        base = state(names)
        for T in counts:
            cands = candidates(e, op.op, T)
            total += len(cands)
            status = [None] * len(cands)
            for first, count in ranges_for(T, share, N):
                if first == 0:   # the check sees a run that writes nothing: poison alone is not what the step wrote
                    assert run(e, op.op, T, -1, first, count, capi.RUN_POISON_ONLY) == capi.OK
                    assert not same(state(names), base), (op.layer, T, "poisoning the output is invisible")
                assert run(e, op.op, T, -1, first, count) == capi.OK
                assert same(state(names), base), (op.layer, T, first, count, "the engine's own choice differs from its step")
                for i, cd in enumerate(cands):
                    rc = run(e, op.op, T, i, first, count)
                    st = "declined" if rc == capi.DECLINED else "ran"
                    if status[i] not in (None, st):
                        failures.append((op.layer.decode(), T, cd.name.decode(), first, count, "declined on some ranges only"))
                    status[i] = st
                    if st == "declined":     # (its output range was poisoned all the same)
                        assert run(e, op.op, T, -1, first, count) == capi.OK
                    elif not same(state(names), base):
                        failures.append((op.layer.decode(), T, cd.name.decode(), first, count, "output differs"))
                        for f in range(0, N, share):        # put the step's values back
                            run(e, op.op, share, -1, f, min(share, N - f))
                        assert same(state(names), base)
            checked += status.count("ran")
            declined += status.count("declined")
        for s in (ref_slots if ref_slots is not None else check_slots):
            r = layer_ratio(e, op, table, s, cache)
            worst[op.layer.decode()] = max(worst.get(op.layer.decode(), 0.0), r)
    # a fresh step after the sweep is what it was before it
    e.submit(0, N)
    e.wait()
    for s in range(N):
        assert np.array_equal(e.read_head(s), heads0[s]), s
        r0, r1 = raws0[s], e.read_raw(s)
        assert r0["num_dets"] == r1["num_dets"] and np.array_equal(r0["boxes"], r1["boxes"]) and np.array_equal(r0["scores"], r1["scores"])
    for layer, r in worst.items():
        log(f"  {layer:24s} worst err/bound {r:.3f}")
    return checked, declined, total, worst, failures


def ipws_all(e, ops, counts):
    """Every images-per-workgroup value the engine's candidates use (the pointwise kernel's ipw counts channel blocks)."""
    return sorted({c.ipw for op in ops for T in counts for c in candidates(e, op.op, T) if c.ipw > 1 and not (c.flags & 8)})


def _report(tag, res, t0, capsys):
    checked, declined, total, worst, failures = res
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    with capsys.disabled():
        print(f"\n[conv candidates {tag}] {checked} (op, count, candidate) triples checked bitwise, {declined} declined by run_conv, "
              f"{total} listed; worst layer err/bound {', '.join(f'{k} {v:.3f}' for k, v in top)}; {time.time() - t0:.1f} s")
    assert not failures, failures[:10]
    assert checked + declined == total and checked > 0
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def _post_exact(e, net):
    """decode / NMS bit-exact against the oracle on the engine's own heads (the anchor count follows the net size)."""
    for s in range(e.num_slots):
        head = e.read_head(s)
        assert head.shape[0] == sum((net // st) ** 2 for st in (8, 16, 32))
        raw, exp = e.read_raw(s), oracle.decode_nms(head, net, 14, 8)
        assert raw["num_dets"] == exp["num_dets"] and np.array_equal(raw["anchors"], exp["anchors"])
        assert np.array_equal(raw["boxes"], exp["boxes"]) and np.array_equal(raw["scores"], exp["scores"])
        assert np.array_equal(raw["kpts"], exp["kpts"])


CONFIGS = [   # (id, net, slots, backbone / dtype)
    ("640x1", 640, 1, "c2f"),
    ("640x7", 640, 7, "c2f"),
    ("416x7", 416, 7, "c2f"),
    ("96x5", 96, 5, "c2f"),
    ("224x5", 224, 5, "c2f"),
    ("1024x2", 1024, 2, "c2f"),
    ("shufflenet-int8-416x4", 416, 4, "shuffle-int8"),
    ("64x3", 64, 3, "c2f"),                # the smallest net: P5 2 x 2, P4 4 x 4 -- every pixel a border pixel
]


@pytest.mark.parametrize("tag,net,slots,kind", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_conv_candidate_is_bitwise_the_choice_and_within_the_bound(blob, capsys, tag, net, slots, kind):
    t0 = time.time()
    b = blob if kind == "c2f" else weights.quantize_blob_int8(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE))
    lines = []
    with YoloEngine(None, (1280, 1024), weights_blob=b, net_size=net, num_slots=slots) as e:
        load_frames(e, slots)
        res = sweep(e, b, lines.append)
        if net in (64, 96, 224, 1024):
            _post_exact(e, net)
    with capsys.disabled():
        print("\n".join(lines))
    _report(tag, res, t0, capsys)


def test_slow_every_conv_candidate_on_a_256_slot_engine(blob, capsys):
    """The slow case: two stream shares of 128, where the resident-weight, ipw = 4 and multi-block pointwise candidates
    live.  Bitwise checks and the bound on sampled slots (first, last, both sides of every ipw boundary)."""
    t0 = time.time()
    lines = []
    with YoloEngine(None, (1280, 1024), weights_blob=blob, net_size=320, num_slots=256) as e:
        load_frames(e, 256)
        res = sweep(e, blob, lines.append, ref_slots=[0, 1, 3, 4, 127, 128, 255])
    with capsys.disabled():
        print("\n".join(lines))
    _report("320x256", res, t0, capsys)


def test_slow_every_conv_candidate_on_a_2048_engine(blob, capsys):
    """The largest net irmv_engine_create accepts: 256 x 256 at stride 8, 86016 anchors; decode / NMS bit-exact too."""
    t0 = time.time()
    lines = []
    with YoloEngine(None, (1280, 1024), weights_blob=blob, net_size=2048, num_slots=1) as e:
        load_frames(e, 1)
        res = sweep(e, blob, lines.append)
        _post_exact(e, 2048)
    with capsys.disabled():
        print("\n".join(lines))
    _report("2048x1", res, t0, capsys)


def test_per_layer_check_sees_what_the_end_to_end_bounds_miss(blob, onet, frame0, capsys):
    """One weight of model.8.m.0.cv1 moved by 0.02 in a copy of the blob: the engine built from it still passes the end to
    end tolerances against the oracle of the ORIGINAL blob, while the per-layer check flags that layer and no other."""
    hdr, layers = weights.parse_blob(blob)
    specs, tensors = [], []
    for sp, w, b in layers:
        w = w.copy()
        if sp.name == "model.8.m.0.cv1":
            w[5, 1, 1, 7] = np.float16(float(w[5, 1, 1, 7]) + 0.02)
        specs.append(sp)
        tensors.append((w, b.copy()))
    bad = weights.build_blob(specs, tensors, hdr["nc"], hdr["nk"], hdr["backbone"])
    table = layer_table(blob)                      # the reference: the original weights
    x = oracle.preprocess(frame0, 640)
    with YoloEngine(None, (1280, 1024), weights_blob=bad) as e:
        e.get_src_image_buffer(0)[:] = frame0
        e.detect(0)
        for tap in ("8", "9", "12", "15", "21"):
            _, t_o = onet.forward(x, emulate_fp16=True, tap=tap)
            t_g = e.read_tap(tap, 0)
            assert np.abs(t_g - t_o).max() <= EMU_TOL and np.abs(t_g - t_o).mean() <= 2e-3, tap
        head_err = float(np.abs(e.read_head(0) - onet.forward(x)).max())
        assert head_err <= HEAD_TOL
        ops = conv_ops(e)
        e.read_tap(next(op.out_tensor.decode() for op in ops if op.out_lazy), 0)   # the layers fused kernels keep on chip, recomputed
        cache, ratios = {}, {}
        for op in ops:
            own_values(e, op, ops, 1, cache)
            ratios[op.layer.decode()] = layer_ratio(e, op, table, 0, cache)
    flagged = sorted(k for k, v in ratios.items() if v > 1.0)
    with capsys.disabled():
        print(f"\n[sensitivity] head max|d| {head_err:.4f} (HEAD_TOL {HEAD_TOL}); model.8.m.0.cv1 err/bound "
              f"{ratios['model.8.m.0.cv1']:.1f}; next worst {max(v for k, v in ratios.items() if k != 'model.8.m.0.cv1'):.3f}")
    assert flagged == ["model.8.m.0.cv1"], flagged
