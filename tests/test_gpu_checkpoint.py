"""The engine on a BN-folded checkpoint (tests/checkpoint.py) that came in through a real protobuf file and the importer.

Every weight the other GPU tests run is i.i.d. Gaussian with one gain per layer (weights.synthetic_tensors), or crafted
Detect finals.  This blob has per-channel scales over four orders of magnitude, dead channels, negative gains, biases far
above sum |w x| and 16 % of its weights in the fp16 subnormal range.  The per-element bound of
tests/test_gpu_conv_candidates.py scales with each channel's own |b| + sum |w||x|, so it is used as it stands: sweep(),
_report(), _post_exact(), M_REL and C_ACC are that module's.

  1. the per-layer sweep (every candidate bitwise the engine's choice, every layer within bound()) on a batched 64 x 64
     engine and on the single-frame plan at 224, where the fused c2f2 / c2f32 / bneck64 / kpt3 kernels and the grouped
     Detect heads run;
  2. dead output channels (w' = 0, so the output is silu(b') whatever the input holds, as long as it is finite): the stored
     bits are one value at every pixel of every slot, within the bound of silu(b');
  3. the int8 load path on q * scale that are fp16 subnormals and rounding ties (engine_graph.cpp float_to_half_bits
     against NumPy's cast);
  4. the head distance engine vs oracle, printed (HEAD_TOL is a statement about the synthetic blob; DESIGN.md has the figure).
"""
import time

import numpy as np
import pytest

import checkpoint
import conv_ref
import test_gpu_conv_candidates as cc
from irmv_detection_amd import frames, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle

pytestmark = pytest.mark.gpu

NET = 96          # the checkpoint's calibration size


@pytest.fixture(scope="module")
def ck_blob():
    return checkpoint.imported_blob(0)


def dead_channel_check(e, blob):
    """-> (ops checked, channels checked, worst err / bound).  e has run a step on all its slots."""
    N = e.num_slots
    ops = cc.conv_ops(e)
    table = cc.layer_table(blob)
    lazy = sorted({op.out_tensor.decode() for op in ops if op.out_lazy})
    if lazy:
        for s in range(N):
            e.read_tap(lazy[0], s)                    # the layers fused kernels keep on chip, recomputed
    share = -(-N // e.num_streams)
    n_ops = n_ch = 0
    worst = 0.0
    for op in ops:
        w, b = table[op.layer.decode()]
        assert len(w) == op.cout
        dead = np.flatnonzero(~w.reshape(len(w), -1).any(axis=1))
        if op.res.C or op.out_f32 or not len(dead):
            continue
        cc.own_values(e, op, ops, share, {})
        for seg in (op.s0, op.s1):
            if seg.C:
                x = conv_ref.decode(cc.read(e, seg.tensor.decode(), 0, N), seg.tensor.decode())[..., seg.coff:seg.coff + seg.C]
                assert np.isfinite(x).all(), (op.layer, seg.tensor)
        raw = cc.read(e, op.out_tensor.decode(), 0, N)[..., op.out_coff:op.out_coff + op.cout]
        val = conv_ref.decode(raw, op.out_tensor.decode()).astype(np.float64)
        for c in dead:
            bits = np.unique(raw[..., c])
            assert len(bits) == 1, (op.layer.decode(), int(c), [hex(v) for v in bits[:8]])
            z = float(b[c])
            y = conv_ref.silu(np.float64(z)) if op.act == 1 else z
            r = abs(float(val[0, 0, 0, c]) - y) / cc.bound(np.float64(y), abs(z), False)
            assert r <= 1.0, (op.layer.decode(), int(c), z, float(val[0, 0, 0, c]), y)
            worst = max(worst, float(r))
        n_ops += 1
        n_ch += len(dead)
    return n_ops, n_ch, worst


@pytest.mark.parametrize("tag,net,slots", [("64x3", 64, 3), ("224x1", 224, 1)])
def test_checkpoint_every_conv_candidate_is_bitwise_the_choice_and_within_the_bound(ck_blob, capsys, tag, net, slots):
    t0 = time.time()
    lines = []
    with YoloEngine(None, (1280, 1024), weights_blob=ck_blob, net_size=net, num_slots=slots) as e:
        cc.load_frames(e, slots)
        res = cc.sweep(e, ck_blob, lines.append)
        cc._post_exact(e, net)
        n_ops, n_ch, worst = dead_channel_check(e, ck_blob)
    with capsys.disabled():
        print("\n".join(lines))
        print(f"[checkpoint {tag}] dead channels: {n_ch} of {n_ops} ops one bit pattern each, worst err/bound {worst:.3f}")
    assert n_ops >= 20 and n_ch >= 40
    cc._report("checkpoint " + tag, res, t0, capsys)


@pytest.fixture(scope="module")
def engine96(ck_blob):
    """Four slots at the calibration size, the four calibration frames, one step."""
    with YoloEngine(None, (1280, 1024), weights_blob=ck_blob, net_size=NET, num_slots=checkpoint.N_CALIB) as e:
        cc.load_frames(e, checkpoint.N_CALIB)
        e.submit(0, checkpoint.N_CALIB)
        e.wait()
        yield e


def test_dead_channels_hold_one_value_everywhere(engine96, ck_blob, capsys):
    n_ops, n_ch, worst = dead_channel_check(engine96, ck_blob)
    with capsys.disabled():
        print(f"\n[checkpoint 96x4] dead channels: {n_ch} of {n_ops} ops one bit pattern each, worst err/bound {worst:.3f}")
    assert n_ops >= 20 and n_ch >= 40


def test_head_distance_engine_vs_oracle(engine96, ck_blob, capsys):
    """Printed, not bounded: HEAD_TOL (tests/test_gpu_engine.py) was set on the synthetic blob.  What is asserted is what
    does not depend on the weights: the post stage on the engine's own head is the oracle's bit for bit, and the head is finite."""
    onet = oracle.Net(ck_blob)
    dist, ncand = [], []
    for s in range(checkpoint.N_CALIB):
        head = engine96.read_head(s)
        assert np.isfinite(head).all()
        ho = onet.forward(oracle.preprocess(frames.synthetic_frame(s), NET))
        dist.append(float(np.abs(head - ho).max()))
        ncand.append(oracle.decode_nms(head, NET, 14, 8)["n_candidates"])
    cc._post_exact(engine96, NET)
    with capsys.disabled():
        print(f"\n[checkpoint 96x4] head max|d| engine vs oracle.Net(blob): {', '.join(f'{d:.3e}' for d in dist)}; candidates {ncand}")
    assert min(ncand) >= 1


def test_int8_checkpoint_equals_its_python_dequantisation(capsys):
    """test_engine_int8_blob_equals_dequantised_fp16_blob (tests/test_int8_weights.py) on q * scale that reach the subnormal
    branch of float_to_half_bits and its ties."""
    from test_int8_weights import _dequantised_fp16_blob
    b8, layer, c = checkpoint.int8_blob_with_ties(0)
    n_sub, n_tie, n_sub_tie = checkpoint.int8_products(b8)
    assert n_sub >= 1 and n_tie >= 1 and n_sub_tie >= 128
    heads = []
    for b in (b8, _dequantised_fp16_blob(b8)):
        with YoloEngine(None, (1280, 1024), weights_blob=b, net_size=NET) as e:
            e.get_src_image_buffer()[:] = frames.synthetic_frame(1)
            e.detect()
            head, raw = e.read_head(0).copy(), e.read_raw(0)
            ops = cc.conv_ops(e)
            lazy = sorted({op.out_tensor.decode() for op in ops if op.out_lazy})
            if lazy:
                e.read_tap(lazy[0], 0)
            op = next(o for o in ops if o.layer.decode() == layer)
            heads.append((head, raw, cc.read(e, op.out_tensor.decode(), 0, 1)[0, ..., op.out_coff + c]))
    assert np.array_equal(heads[0][0], heads[1][0]) and np.array_equal(heads[0][2], heads[1][2])
    # the hand-made channel is seen: bias 0 and weights of a few steps of 2^-24 leave an output of a few fp16 subnormal steps
    assert len(np.unique(heads[0][2])) >= 4 and int((heads[0][2] & 0x7fff).max()) < 0x0400
    r0, r1 = heads[0][1], heads[1][1]
    assert r0["num_dets"] == r1["num_dets"] and np.array_equal(r0["boxes"], r1["boxes"]) and np.array_equal(r0["scores"], r1["scores"])
    assert np.array_equal(r0["anchors"], r1["anchors"]) and np.array_equal(r0["kpts"], r1["kpts"])
    d = oracle.decode_nms(heads[0][0], NET, 14, 8)
    assert d["num_dets"] == r0["num_dets"] and np.array_equal(d["boxes"], r0["boxes"])
    with capsys.disabled():
        print(f"\n[checkpoint int8] {n_sub} subnormal q*scale, {n_tie} on a rounding tie ({n_sub_tie} of them subnormal, "
              f"{layer} channel {c} by hand); {r0['num_dets']} detections, heads bitwise equal")
