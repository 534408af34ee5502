"""The graph's layer ops that are not convs -- model.0.conv, the SPPF pools, the depthwise convs and the channel shuffles of
the ShuffleNet backbone -- each run on its own through the C ABI's test hooks (irmv_engine_ops / irmv_engine_run_op) and
checked against tests/conv_ref.py.  The conv sweep (tests/test_gpu_conv_candidates.py) feeds every conv's reference from
the engine's own input tensors, so a wrong value written by one of these kernels would be copied into the next conv's
reference and pass there; here each gets a reference of its own.

For every engine: distinct synthetic frames, one step, then

  * completeness: every op of irmv_engine_ops that writes an activation tensor is a conv (the sweep), a fused kernel
    (asserted bitwise against its layers inside the sweep), the preprocess (bit-exact tests of tests/test_gpu_engine.py
    and tests/test_gpu_rect.py), or one of the four kinds checked here -- and the number of those matches the graph;
  * bitwise against the step, on every slot range production launches (each stream share, one slot, the last slot):
    a poison-only run (NaN over the op's output channels on its slots) is visible and touches nothing else, the op's own
    run after the poison gives back the step's output, and nothing outside its output channels and slots moves;
  * the reference, on the engine's own input tensors:
      model.0.conv   the per-layer bound of tests/test_gpu_conv_candidates.py (bound()) on channels 0-2 of "input", and
                     channel 3 of "input" is +0 everywhere (conv0_kernel multiplies it by zero weights: a NaN or an Inf
                     there would poison every output);
      depthwise      the same bound (the bias is scaled by log2 e in fp64 and rounded to fp32: the acc term covers it);
      shuffle        bitwise on the raw fp16 bits;
      pool           exact: every value equals the reference pooled from the step's own channels [0, C) of "9.cat",
                     compared as fp16 values (-0 == +0) and bitwise wherever the value is not zero.  Of two zeros of
                     different sign, v_pk_max_f16 may return either (k_conv.hip, hmax8), and the LDS and global kernels
                     may pick different ones; no later layer can tell them apart, so the sign of a zero is not checked
                     (the same holds for the pool's comparison with the step).

Two kinds that are covered elsewhere have a sweep of their own over source geometries, tests/test_gpu_input_geometry.py:

  * front: bitwise against preprocess + model.0.conv + model.1.conv on every path of the front kernel and every tile class;
  * pre: bitwise against the oracle's preprocess on the same zoo.

The engines reach all four SPPF variants (irmv_sppf_slab: LDS slabs of 8, 16 and 32 channels, and the global-memory
kernel of P5 maps above 2400 pixels), P5 maps from 2 x 2 to 64 x 64, 64 x 2 and 2 x 64, and every depthwise (stride 1
and 2) and shuffle op of the ShuffleNet backbone, fp16 and int8, on maps down to 13 x 11.  The 1568 and 2048 engines
are the slow cases (test_slow_...; leave them out with -k "not slow").
"""
import ctypes as C
import time

import numpy as np
import pytest

import conv_ref
from irmv_detection_amd import arch, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_gpu_conv_candidates import EMU_TOL, HEAD_TOL, bound, layer_table, load_frames, read

pytestmark = pytest.mark.gpu

CHECKED = ("conv0", "pool", "dw", "shuffle")
COVERED = {   # the other kinds that write activation tensors, and where they are checked
    "conv": "the sweep of tests/test_gpu_conv_candidates.py",
    "front": "bitwise against its layers in the sweep, and on the zoo of tests/test_gpu_input_geometry.py", "c2f2": "bitwise against its layers in the sweep",
    "c2f32": "bitwise against its layers in the sweep", "bneck": "bitwise against its layers in the sweep",
    "kpt3": "bitwise against its layers in the sweep",   # (all four also alone, on written inputs: tests/test_gpu_act_craft.py)
    "boxg": "alone, on written candidates and activations: tests/test_gpu_gather_craft.py (here: check_boxg)",
    "pre": "the preprocess bit-exact tests of tests/test_gpu_engine.py and tests/test_gpu_rect.py, and bitwise against the oracle "
           "on the zoo of tests/test_gpu_input_geometry.py",
}
P5_C = 128   # model.9.m: channels per slice of 9.cat


# ---- the hooks --------------------------------------------------------------------------------------------------
def graph_ops(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_ops(e._h, None, 0, C.byref(n)))
    arr = (capi.GraphOp * n.value)()
    capi.check(e._L.irmv_engine_ops(e._h, arr, n.value, C.byref(n)))
    return list(arr)


def run_op(e, op, first, count, flags=capi.RUN_POISON):
    """Every run first fills the channels it must write with NaN (capi.RUN_POISON)."""
    capi.check(e._L.irmv_engine_run_op(e._h, op, first, count, flags))


def sppf_slab(count, H, W):
    return capi.load().irmv_sppf_slab(count, H, W, P5_C)


def f16(raw):
    return raw.view(np.float16)


# ---- the pieces of the check ---------------------------------------------------------------------------------------
def slot_ranges(N, share, extra=()):
    """Every slot range production launches an op on: each stream share, one slot, the last slot (and `extra`)."""
    r = [(f, min(share, N - f)) for f in range(0, N, share)] + [(0, 1), (N - 1, 1)] + list(extra)
    return list(dict.fromkeys(r))


def same_values(a, b, pool):
    """Bitwise; a pool's zeros compare as values (see the module docstring)."""
    if not pool:
        return np.array_equal(a, b)
    return bool(((f16(a) == f16(b)) & ((a == b) | (f16(a) == 0))).all())


def check_runs(e, op, ranges):
    """The op's own run on every range against what the step left."""
    N = e.num_slots
    out, lo, hi = op.out_tensor.decode(), op.out_coff, op.out_coff + op.out_C
    inputs = sorted({s.tensor.decode() for s in (op.s0, op.s1)} - {"", out})
    base = read(e, out, 0, N)
    base_in = {n: read(e, n, 0, N) for n in inputs}
    pool = op.kind == b"pool"
    for i, (first, count) in enumerate(ranges):
        if i == 0:   # poison alone: exactly the op's channels on its slots turn NaN -- a run that writes nothing is seen
            run_op(e, op.op, first, count, capi.RUN_POISON_ONLY)
            got = read(e, out, 0, N)
            assert (got[first:first + count, ..., lo:hi] == 0xFFFF).all(), (op.layer, "poison missed part of the output")
            assert not same_values(got, base, pool), (op.layer, "poisoning the output is invisible")
            got[first:first + count, ..., lo:hi] = base[first:first + count, ..., lo:hi]
            assert np.array_equal(got, base), (op.layer, "poison outside the op's output")
        run_op(e, op.op, first, count)
        got = read(e, out, 0, N)
        assert same_values(got, base, pool), (op.layer.decode(), first, count, "the op's own run differs from the step")
        for n, v in base_in.items():
            assert np.array_equal(read(e, n, 0, N), v), (op.layer.decode(), first, count, f"input {n} changed")


def check_boxg(e, op, ranges):
    """A candidate gather op (it names no output tensor of its own: it writes head rows at candidate anchors).
    irmv_engine_op_io describes it -- its level's three box convs, the level input, the head's box channels (and the keypoint
    channels where that branch rides) -- and on the bitmap a step leaves behind, all zero, its run on every range builds empty
    lists and writes nothing: the dense head is what it was.  An engine without the sparse head refuses the run."""
    N = e.num_slots
    io = capi.OpIo()
    capi.check(e._L.irmv_engine_op_io(e._h, op.op, C.byref(io)))
    lv = int(op.layer.decode().split(".")[3])
    assert op.layer.decode() == f"model.22.cv2.{lv}.g" and op.kname.decode().startswith("box_gather_c") and not op.out_tensor
    assert io.n_sub == 3 and io.n_reads == 1 and io.n_writes in (1, 2)
    head = io.writes[0].tensor.decode()
    assert (head, io.writes[0].coff, io.writes[0].C) == (f"head.{lv}", 0, 64)
    if io.n_writes == 2:
        assert (io.writes[1].tensor.decode(), io.writes[1].coff, io.writes[1].C) == (head, 80, 16)
    sparse, _ = e.debug_cand_bits(0)
    if not sparse:
        assert e._L.irmv_engine_run_op(e._h, op.op, 0, 1, 0) == capi.ERR_ARG
        return
    base = read(e, head, 0, N)
    for first, count in ranges:
        assert not any(e.debug_cand_bits(s)[1].any() for s in range(first, first + count))
        run_op(e, op.op, first, count, 0)
    assert np.array_equal(read(e, head, 0, N).view(np.uint32), base.view(np.uint32)), (op.layer, "a run without a candidate wrote head rows")


def ref_ratio(e, op, table, specs, slot):
    """conv0, dw: worst err / bound of the op's output on one slot.  shuffle, pool: the number of mismatches (must be 0)."""
    out_name = op.out_tensor.decode()
    out = read(e, out_name, slot, 1)[0][..., op.out_coff:op.out_coff + op.out_C]
    s0 = op.s0.tensor.decode()
    x_raw = read(e, s0, slot, 1)[0][..., op.s0.coff:op.s0.coff + op.s0.C]
    kind = op.kind.decode()
    if kind == "conv0":
        assert s0 == "input" and x_raw.shape[-1] == 4
        assert (x_raw[..., 3] == 0).all(), "channel 3 of input is not +0 everywhere"
        w, b = table["model.0.conv"]
        y, acc = conv_ref.conv0(conv_ref.decode(x_raw, "input"), w, b)
        return float((np.abs(conv_ref.decode(out, out_name) - y) / bound(y, acc, False)).max())
    if kind == "dw":
        layer = op.layer.decode()
        w, b = table[layer]
        y, acc = conv_ref.dwconv(conv_ref.decode(x_raw, s0), w, b, specs[layer].stride)
        assert y.shape == out.shape, layer
        return float((np.abs(conv_ref.decode(out, out_name) - y) / bound(y, acc, False)).max())
    if kind == "shuffle":
        b_raw = read(e, op.s1.tensor.decode(), slot, 1)[0][..., op.s1.coff:op.s1.coff + op.s1.C]
        return float(np.count_nonzero(out != conv_ref.shuffle(x_raw, b_raw)))
    assert kind == "pool" and x_raw.shape[-1] == P5_C and out.shape[-1] == 3 * P5_C
    want = np.concatenate(conv_ref.sppf(f16(x_raw).astype(np.float64)), axis=-1)
    bits = want.astype(np.float16).view(np.uint16)
    return float(np.count_nonzero((f16(out).astype(np.float64) != want) | ((want != 0) & (out != bits))))


def failing(kind, ratio):
    return ratio > 1.0 if kind in ("conv0", "dw") else ratio != 0


def check_graph(e, blob, log, tag, ranges, ref_slots, slabs, shuffle):
    """The whole check on engine e (frames loaded, nothing in flight); returns {layer: worst ratio}."""
    t0 = time.time()
    N = e.num_slots
    e.submit(0, N)
    e.wait()
    ops = graph_ops(e)
    for o in ops:
        if o.out_tensor:
            assert o.kind.decode() in CHECKED + tuple(COVERED), (o.kind, o.layer, "an op kind nobody checks writes an activation tensor")
    mine = [o for o in ops if o.kind.decode() in CHECKED]
    kind_of = {o.layer.decode(): o.kind.decode() for o in mine}
    counts = {k: sum(o.kind.decode() == k for o in mine) for k in CHECKED}
    assert counts == {"conv0": 1, "pool": 1, "dw": 10 if shuffle else 0, "shuffle": 7 if shuffle else 0}, counts
    for s in range(N):   # under the fused front, "input" and "0" are kept on chip: recompute them on every slot, as sweep() does
        e.read_tap("0", s)
    specs = {sp.name: sp for sp, _, _ in weights.parse_blob(blob)[1]}
    table = layer_table(blob)
    worst = {}
    for op in mine:
        check_runs(e, op, ranges)
        worst[op.layer.decode()] = max(ref_ratio(e, op, table, specs, s) for s in ref_slots)
    for op in ops:
        if op.kind == b"boxg":
            check_boxg(e, op, ranges)
    parts = []
    for k in CHECKED:
        w = [(v, n) for n, v in worst.items() if kind_of[n] == k]
        if w:
            v, n = max(w)
            parts.append(f"{k} {n} " + (f"err/bound {v:.3f}" if k in ("conv0", "dw") else f"{int(v)} mismatches"))
    log(f"[graph ops {tag}] checked {counts}; SPPF slab(s) {sorted(slabs)} (0: global kernel); worst {', '.join(parts)}; "
        f"{len(ranges)} slot ranges, {time.time() - t0:.1f} s")
    bad = {n: v for n, v in worst.items() if failing(kind_of[n], v)}
    assert not bad, bad
    return worst


def _run(blob, capsys, tag, W, H, slots, shuffle=False, slabs=(8,), src=(1280, 1024), extra_ranges=(), ref_slots=None, **kw):
    lines = []
    with YoloEngine(None, src, weights_blob=blob, net_size=W, net_height=H, num_slots=slots, **kw) as e:
        assert (e.net_width, e.net_height) == (W, H)
        share = -(-slots // e.num_streams)
        ranges = slot_ranges(slots, share, extra_ranges)
        ran = {sppf_slab(count, H // 32, W // 32) for _, count in ranges}     # the intended SPPF variants, before relying on them
        assert ran == set(slabs), (ran, slabs)
        for s in range(slots):   # distinct frames (cropped to a small source)
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(3 + s)[:src[1], :src[0]]
        worst = check_graph(e, blob, lines.append, tag, ranges, ref_slots if ref_slots is not None else list(range(slots)), ran, shuffle)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    return worst


def _sblob(int8):
    b = weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)
    return weights.quantize_blob_int8(b) if int8 else b


# ---- the engines -----------------------------------------------------------------------------------------------------
SQUARE = [   # (id, net, slots): slab 8 on P5 maps 20^2, 13^2, 3^2 and 2^2 (every pixel a border pixel)
    ("640x1", 640, 1), ("416x3", 416, 3), ("96x5", 96, 5), ("64x3", 64, 3),
]


@pytest.mark.parametrize("tag,net,slots", SQUARE, ids=[c[0] for c in SQUARE])
def test_graph_ops_square(blob, capsys, tag, net, slots):
    _run(blob, capsys, tag, net, net, slots)


RECT = [   # (id, W, H, slots): P5 maps 16 x 20, 2 x 64 and 64 x 2 (rows x columns)
    ("640x512x2", 640, 512, 2), ("2048x64x1", 2048, 64, 1), ("64x2048x1", 64, 2048, 1),
]


@pytest.mark.parametrize("tag,W,H,slots", RECT, ids=[c[0] for c in RECT])
def test_graph_ops_rect(blob, capsys, tag, W, H, slots):
    _run(blob, capsys, tag, W, H, slots)


SHUFFLE = [   # (id, W, H, slots, int8): every dw (stride 1 and 2) and shuffle op, maps down to 13 x 11
    ("shufflenet-fp16-640x1", 640, 640, 1, False), ("shufflenet-int8-416x4", 416, 416, 4, True),
    ("shufflenet-int8-416x352x2", 416, 352, 2, True),
]


@pytest.mark.parametrize("tag,W,H,slots,int8", SHUFFLE, ids=[c[0] for c in SHUFFLE])
def test_graph_ops_shufflenet(capsys, tag, W, H, slots, int8):
    _run(_sblob(int8), capsys, tag, W, H, slots, shuffle=True)


def test_graph_ops_all_three_sppf_slabs_in_one_engine(blob, capsys):
    """64 net, 192 slots on one stream: run_op counts 192, 96 and 1 take the LDS kernel with slabs of 32, 16 and 8
    channels (192 * 128 / 32 = 96 * 128 / 16 = 768 workgroups)."""
    _run(blob, capsys, "64x192", 64, 64, 192, slabs=(32, 16, 8), src=(128, 128), num_streams=1,
         extra_ranges=[(0, 96), (96, 96), (95, 96)], ref_slots=[0, 1, 95, 96, 191])


@pytest.mark.parametrize("net", [1568, 2048])
def test_slow_graph_ops_global_sppf_kernel(blob, capsys, net):
    """P5 maps of 49 x 49 and 64 x 64 pixels do not fit an LDS slab: the global-memory sppf_pool_kernel."""
    _run(blob, capsys, f"{net}x1", net, net, 1, slabs=(0,))


# ---- sensitivity ---------------------------------------------------------------------------------------------------
def _moved(blob, layer, idx, delta):
    hdr, layers = weights.parse_blob(blob)
    specs, tensors = [], []
    for sp, w, b in layers:
        w = w.copy()
        if sp.name == layer:
            w[idx] = np.float16(float(w[idx]) + delta)
        specs.append(sp)
        tensors.append((w, b.copy()))
    return weights.build_blob(specs, tensors, hdr["nc"], hdr["nk"], hdr["backbone"])


def _sensitivity(good, layer, idx, delta, taps, frame0, capsys):
    """The engine of a blob with one weight of `layer` moved by delta: its taps and head still pass the end to end
    tolerances against the oracle of the ORIGINAL blob, while the per-op check (against the original weights) flags that
    layer and no other."""
    bad = _moved(good, layer, idx, delta)
    on = oracle.Net(good)
    x = oracle.preprocess(frame0, 640)
    table = layer_table(good)
    specs = {sp.name: sp for sp, _, _ in weights.parse_blob(good)[1]}
    tap_err = 0.0
    with YoloEngine(None, (1280, 1024), weights_blob=bad) as e:
        e.get_src_image_buffer(0)[:] = frame0
        e.detect(0)
        for tap in taps:
            _, t_o = on.forward(x, emulate_fp16=True, tap=tap)
            d = np.abs(e.read_tap(tap, 0) - t_o)
            tap_err = max(tap_err, float(d.max()))
            assert d.max() <= EMU_TOL and d.mean() <= 2e-3, tap
        head_err = float(np.abs(e.read_head(0) - on.forward(x)).max())
        assert head_err <= HEAD_TOL
        e.read_tap("0", 0)
        mine = [o for o in graph_ops(e) if o.kind.decode() in CHECKED]
        ratios = {o.layer.decode(): (o.kind.decode(), ref_ratio(e, o, table, specs, 0)) for o in mine}
    flagged = sorted(n for n, (k, v) in ratios.items() if failing(k, v))
    with capsys.disabled():
        print(f"\n[graph ops sensitivity] {layer}{list(idx)} + {delta}: worst tap max|d| {tap_err:.4f} (EMU_TOL {EMU_TOL}), head "
              f"{head_err:.4f} (HEAD_TOL {HEAD_TOL}); {layer} err/bound {ratios[layer][1]:.1f}; next worst err/bound "
              f"{max([v for n, (k, v) in ratios.items() if n != layer and k in ('conv0', 'dw')], default=0):.3f}")
    assert flagged == [layer], flagged


def test_per_op_check_sees_a_moved_model0_weight(blob, frame0, capsys):
    """One weight of model.0.conv moved by 0.008 (measured on frame 0: worst tap max|d| 0.028 of EMU_TOL 0.06, head 0.028
    of HEAD_TOL 0.04; model.0.conv err/bound 8.3, the pool 0 mismatches)."""
    _sensitivity(blob, "model.0.conv", (5, 1, 1, 1), 0.008, ("1", "2", "8", "9", "15", "21"), frame0, capsys)


def test_per_op_check_sees_a_moved_depthwise_weight(frame0, capsys):
    """One weight of model.5.b2.dw (ShuffleNet, fp16 blob) moved by 0.005 (measured on frame 0: worst tap max|d| 0.019 of
    EMU_TOL 0.06, head 0.021 of HEAD_TOL 0.04; model.5.b2.dw err/bound 80, the next worst dw layer 0.80).  At 0.02 the
    head came to 0.0399: a fourfold larger move is about all the end to end bound still lets through."""
    _sensitivity(_sblob(False), "model.5.b2.dw", (7, 1, 1, 0), 0.005, ("4", "5", "6", "8", "9", "15", "21"), frame0, capsys)


@pytest.mark.parametrize("net", [64, 416])
def test_pool_data_tells_the_classic_pool_bugs_apart(blob, net):
    """The pool's values in the engine's 9.cat differ from a pool with zero padding instead of clipped windows (on both
    maps), and from one with the 9 x 9 and 13 x 13 results swapped on the 13 x 13 map.  On the 2 x 2 map of the 64 net
    every window holds the whole map: p5 = p9 = p13 there, and no data can tell the groups apart."""
    import torch
    import torch.nn.functional as F
    slots = 3
    with YoloEngine(None, (1280, 1024), weights_blob=blob, net_size=net, num_slots=slots) as e:
        load_frames(e, slots, seed0=3)
        e.submit(0, slots)
        e.wait()
        raw = read(e, "9.cat", 0, slots)
    a, out = f16(raw[..., :P5_C]).astype(np.float64), f16(raw[..., P5_C:]).astype(np.float64)
    assert np.array_equal(out, np.stack([np.concatenate(conv_ref.sppf(a[s]), axis=-1) for s in range(slots)]))
    p, zp = torch.from_numpy(a).permute(0, 3, 1, 2), []
    for _ in range(3):      # zero padding: the pools see zeros beyond the border
        p = F.max_pool2d(F.pad(p, (2, 2, 2, 2), value=0.0), 5, 1, 0)
        zp.append(p.permute(0, 2, 3, 1).numpy())
    assert not np.array_equal(out, np.concatenate(zp, axis=-1))
    swapped = np.concatenate([out[..., :P5_C], out[..., 2 * P5_C:], out[..., P5_C:2 * P5_C]], axis=-1)
    assert np.array_equal(out, swapped) == (net == 64)
