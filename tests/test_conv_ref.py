"""tests/conv_ref.py (the per-layer fp64 reference of tests/test_gpu_conv_candidates.py) against torch's conv2d in float64
and against the C oracle's own conv layer, at the shapes the engine hands it: stride 1 / 2, 1x1 / 3x3, a residual, an
upsampled concat, odd map sizes, and a Detect carrier's fused 1x1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref
from irmv_detection_amd import arch, capi, weights
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


# ---- the other ops that write activation tensors (tests/test_gpu_graph_ops.py) -----------------------------------------
@pytest.fixture(scope="module")
def slayers():
    return {sp.name: (sp, w, b) for sp, w, b in weights.parse_blob(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE))[1]}


MAPS = [(1, 1), (2, 2), (3, 3), (13, 11), (64, 2), (2, 64), (7, 5)]


S2_MAPS = [(2, 2), (4, 4), (6, 6), (26, 22), (4, 128), (128, 4)]     # the engine's stride-2 inputs are even; outputs odd too


@pytest.mark.parametrize("name,H,W", [("model.3.b2.dw", H, W) for H, W in MAPS] + [("model.2.b1.dw", H, W) for H, W in S2_MAPS] +
                         [("model.7.b2.dw", 26, 22), ("model.8.b2.dw", 13, 11)])
def test_dwconv_matches_torch(slayers, name, H, W):
    """Depthwise 3x3 against F.conv2d(groups=C), stride 1 (model.3 / model.8) and 2 (model.2 / model.7), onto odd outputs
    too (26 x 22 -> 13 x 11)."""
    sp, w, b = slayers[name]
    assert sp.groups == sp.cout and w.shape == (sp.cout, 3, 3, 1)
    rng = np.random.default_rng(H * 100 + W)
    x = (rng.standard_normal((H, W, sp.cout)) * 2).astype(np.float32)
    y, acc = conv_ref.dwconv(x, w, b, sp.stride)
    xt = torch.from_numpy(x.astype(np.float64)).permute(2, 0, 1)[None]
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    yt = F.conv2d(xt, wt, torch.from_numpy(b.astype(np.float64)), stride=sp.stride, padding=1, groups=sp.cout)[0].permute(1, 2, 0).numpy()
    assert y.shape == yt.shape == (H // sp.stride, W // sp.stride, sp.cout)
    assert np.abs(y - yt).max() <= 1e-12 * max(1.0, acc.max())
    assert (acc >= np.abs(y) - 1e-12).all()
    # acc is |b| + sum |w| |x| over the taps inside the map: the same op on |x|, |w|, |b|
    acc_t = F.conv2d(xt.abs(), wt.abs(), torch.from_numpy(np.abs(b).astype(np.float64)), stride=sp.stride, padding=1, groups=sp.cout)
    assert np.allclose(acc, acc_t[0].permute(1, 2, 0).numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("H,W", MAPS + [(20, 20), (20, 16), (49, 49)])
def test_sppf_matches_chained_max_pools(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    a = rng.standard_normal((H, W, 24)).astype(np.float16)      # fp16 values with ties and both zero signs
    a[rng.random(a.shape) < 0.05] = np.float16(-0.0)
    p5, p9, p13 = conv_ref.sppf(a)
    t = torch.from_numpy(a.astype(np.float64)).permute(2, 0, 1)[None]
    want = []
    for _ in range(3):
        t = F.max_pool2d(t, 5, 1, 2)
        want.append(t[0].permute(1, 2, 0).numpy())
    for got, exp in zip((p5, p9, p13), want):
        assert got.shape == (H, W, 24) and np.array_equal(got, exp)
    # every pool value is one of its window's own values: exact in fp16
    assert np.array_equal(p13.astype(np.float16).astype(np.float64), p13)
    if H >= 13 and W >= 13:      # a pixel whose 13x13 window is whole and whose 5x5 is not its own maximum
        assert (p13 > p9).any() and (p9 > p5).any()


@pytest.mark.parametrize("H,W", [(1, 1), (13, 11), (2, 64)])
def test_shuffle_matches_cat_view_transpose(H, W):
    rng = np.random.default_rng(H + W)
    ta = rng.standard_normal((H, W, 96)).astype(np.float16)
    tb = rng.standard_normal((H, W, 160)).astype(np.float16)
    a, b = ta[..., 32:96], tb[..., 64:128]                     # slices at offsets, as the op records name them
    out = conv_ref.shuffle(a, b)
    x = torch.cat([torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))], dim=-1)   # [H, W, 2 bc]
    x = x.permute(2, 0, 1)[None]
    n, c, h, w = x.shape
    want = x.view(n, 2, c // 2, h, w).transpose(1, 2).reshape(n, c, h, w)[0].permute(1, 2, 0).numpy().astype(np.float16)
    assert out.dtype == np.float16 and np.array_equal(out.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (26, 22), (128, 4), (4, 128)])
def test_conv0_ignores_the_fourth_input_channel(layers, H, W):
    """model.0.conv (3x3 stride 2, 3 -> 16, SiLU) on the engine's 4-channel input: the fourth channel, whatever it holds,
    is no input of the layer.  (The net input is even in both directions; 26 x 22 gives odd outputs.)"""
    sp, w, b = layers["model.0.conv"]
    assert (sp.cin, sp.cout, sp.k, sp.stride, sp.act) == (3, 16, 3, 2, 1)
    rng = np.random.default_rng(H * 7 + W)
    x4 = rng.random((H, W, 4)).astype(np.float32)
    x4[..., 3] = 1e6
    y, acc = conv_ref.conv0(x4, w, b)
    assert y.shape == (H // 2, W // 2, 16)
    yt = _torch(x4[..., :3], w, b, 2, 1)
    assert np.abs(y - yt).max() <= 1e-12 * max(1.0, acc.max())
    x4[..., 3] = 0
    assert np.array_equal(conv_ref.conv0(x4, w, b)[0], y)
