"""tests/conv_ref.py (the per-layer fp64 reference of tests/test_gpu_conv_candidates.py) against torch's conv2d in float64
and against the C oracle's own conv layer, at the shapes the engine hands it: stride 1 / 2, 1x1 / 3x3, a residual, an
upsampled concat, odd map sizes, and a Detect carrier's fused 1x1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref
from irmv_detection_amd import capi, weights
from oracle import oracle


def _torch(x, w, b, stride, act, res=None):
    xt = torch.from_numpy(np.asarray(x, np.float64)).permute(2, 0, 1)[None]
    wt = torch.from_numpy(np.asarray(w, np.float64)).permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, torch.from_numpy(np.asarray(b, np.float64)), stride=stride, padding=w.shape[1] // 2)
    if act == 1:
        y = F.silu(y)
    y = y[0].permute(1, 2, 0).numpy()
    return y if res is None else y + res


def _op(layer, cin, cout, k, stride, act, H, W, s0, s1=None, res=None, out=("out", 0)):
    op = capi.ConvOp()
    op.layer = layer.encode()
    op.ks, op.stride, op.act, op.cin, op.cout, op.cout_pad = k, stride, act, cin, cout, (cout + 15) // 16 * 16
    op.Hin, op.Win, op.Hout, op.Wout = H, W, H // stride, W // stride
    for dst, src in ((op.s0, s0), (op.s1, s1), (op.res, res)):
        if src:
            dst.tensor = src[0].encode()
            dst.coff, dst.C, dst.shift = src[1], src[2], (src[3] if len(src) > 3 else 0)
    op.out_tensor, op.out_coff = out[0].encode(), out[1]
    return op


@pytest.fixture(scope="module")
def layers(blob):
    return {sp.name: (sp, w, b) for sp, w, b in weights.parse_blob(blob)[1]}


@pytest.mark.parametrize("name,H,W", [
    ("model.1.conv", 16, 16),          # 3x3 stride 2, Cin 16
    ("model.3.conv", 14, 10),          # 3x3 stride 2 onto 7 x 5
    ("model.7.conv", 6, 6),            # 3x3 stride 2 onto 3 x 3
    ("model.8.m.0.cv1", 5, 7),         # 3x3 stride 1 on odd maps
    ("model.8.m.0.cv1", 3, 3),         # every tap a border tap
    ("model.8.cv2", 7, 11),            # 1x1
    ("model.22.cv2.0.2", 5, 5),        # 1x1 without activation (Detect final)
])
def test_conv_matches_torch_and_the_oracle(layers, onet, name, H, W):
    sp, w, b = layers[name]
    rng = np.random.default_rng(hash(name) % 1000 + H)
    x = (rng.standard_normal((H, W, sp.cin)) * 2).astype(np.float32)
    y, acc = conv_ref.conv(x, w, b, sp.stride, sp.act)
    assert y.shape == (H // sp.stride, W // sp.stride, sp.cout) and (acc >= np.abs(y) - 1e-12).all()
    yt = _torch(x, w, b, sp.stride, sp.act)
    assert np.abs(y - yt).max() <= 1e-12 * max(1.0, acc.max())
    yo = onet.conv_layer(name, x, sp.cout, sp.stride)          # float32 accumulation
    assert np.abs(y - yo).max() <= 1e-5 * acc.max(), np.abs(y - yo).max()


def test_residual_and_upsampled_concat(layers):
    """The op record's input assembly: s0 a channel slice of a half-resolution tensor read as its nearest 2x upsample,
    s1 a slice of a full-resolution one, and a residual slice added after the activation."""
    sp, w, b = layers["model.12.cv1"]                          # 384 -> 128, 1x1: concat(up(9), 6) at the 16 x 16 level
    rng = np.random.default_rng(5)
    t9 = rng.standard_normal((3, 5, 300)).astype(np.float32)
    t6 = rng.standard_normal((6, 10, 140)).astype(np.float32)
    rt = rng.standard_normal((6, 10, 200)).astype(np.float32)
    op = _op("model.12.cv1", 384, 128, 1, 1, 1, 6, 10, ("9", 20, 256, 1), ("6", 5, 128), res=("r", 40, 128))
    y, acc = conv_ref.op_forward(op, {"9": t9, "6": t6, "r": rt}, w, b)
    up = np.repeat(np.repeat(t9[..., 20:276], 2, axis=0), 2, axis=1)
    x = np.concatenate([up, t6[..., 5:133]], axis=-1)
    xt = torch.from_numpy(t9[..., 20:276].astype(np.float64)).permute(2, 0, 1)[None]
    assert np.array_equal(F.interpolate(xt, scale_factor=2, mode="nearest")[0].permute(1, 2, 0).numpy(), up)
    yt = _torch(x, w, b, 1, 1, rt[..., 40:168])
    assert np.abs(y - yt).max() <= 1e-12 * acc.max()
    assert (acc >= np.abs(rt[..., 40:168])).all()


def test_fused_carrier(layers):
    sp1, w1, b1 = layers["model.22.cv3.1.1"]
    sp2, w2, b2 = layers["model.22.cv3.1.2"]
    rng = np.random.default_rng(9)
    t = rng.standard_normal((7, 7, 64)).astype(np.float32)
    op = _op("model.22.cv3.1.1", 64, 64, 3, 1, 1, 7, 7, ("t", 0, 64))
    y, acc, y2, acc2 = conv_ref.op_forward(op, {"t": t}, w1, b1, (w2, b2))
    assert np.abs(y2 - _torch(_torch(t, w1, b1, 1, 1), w2, b2, 1, 0)).max() <= 1e-12 * acc2.max()
    assert y2.shape == (7, 7, sp2.cout)


def test_decode_is_read_tap_arithmetic():
    h = np.array([1.0, -3.5, 65504.0, 2.0 ** -24], np.float16)
    raw = h.view(np.uint16)
    assert np.array_equal(conv_ref.decode(raw, "input"), h.astype(np.float32))
    assert np.array_equal(conv_ref.decode(raw, "9"), h.astype(np.float32) * np.float32(0.693147180559945309))
