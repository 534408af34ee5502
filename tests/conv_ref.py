"""A plain float64 statement of one conv layer of the engine, built from the engine's own op record (capi.ConvOp).

    input   concat(s0, s1) along channels; a segment with shift 1 is the nearest 2x upsample of its tensor
    conv    k x k, stride s, zero padding k // 2, in im2col form, the blob's fp16 weights as stored (OHWI)
    out     + bias, SiLU if act == 1, + residual (added after the activation)
    fused   a Detect carrier's final 1x1 (bias only) applied to the conv's output

Beside the convs, the other ops of the graph that write activation tensors (tests/test_gpu_graph_ops.py):

    conv0     model.0.conv on the 4-channel "input" tensor: the fourth channel is not an input of the layer
    dwconv    depthwise 3 x 3 (ShuffleNetV2 stages), stride 1 or 2, zero padding 1, bias, no activation
    sppf      the three chained max_pool2d(5, 1, 2) of model.9.m: maxima over clipped windows of radius 2, 4 and 6
    shuffle   concat of two equal-width channel slices + channel shuffle with two groups

The convs also return acc = |b| + sum |w| |x| per output element: the scale of the rounding a float32 accumulation
of that element can make (tests/test_gpu_conv_candidates.py states its bound with it).
"""
from __future__ import annotations

import numpy as np

LN2 = np.float32(0.693147180559945309)


def decode(raw: np.ndarray, name: str) -> np.ndarray:
    """Raw storage of an engine tensor -> the real values irmv_engine_read_tap returns: fp16 activations are stored at the
    log2(e) scale and read back as fp32(h * ln 2); "input" is unscaled; fp32 tensors are what they are."""
    if raw.dtype == np.float32:
        return raw
    f = raw.view(np.float16).astype(np.float32)
    return f if name == "input" else f * LN2


def upsample2(x: np.ndarray) -> np.ndarray:
    return np.repeat(np.repeat(x, 2, axis=0), 2, axis=1)


def segment(t: np.ndarray, coff: int, C: int, shift: int) -> np.ndarray:
    x = t[..., coff:coff + C]
    return upsample2(x) if shift else x


def im2col(x: np.ndarray, k: int, stride: int) -> np.ndarray:
    """[H, W, C] -> [Ho * Wo, k * k * C] in (ky, kx, c) order, zero padding k // 2, Ho = H // stride."""
    H, W, C = x.shape
    Ho, Wo, p = H // stride, W // stride, k // 2
    xp = np.zeros((H + 2 * p, W + 2 * p, C), x.dtype)
    xp[p:p + H, p:p + W] = x
    cols = np.empty((Ho, Wo, k, k, C), x.dtype)
    for ky in range(k):
        for kx in range(k):
            cols[:, :, ky, kx] = xp[ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
    return cols.reshape(Ho * Wo, k * k * C)


def silu(z: np.ndarray) -> np.ndarray:
    return z / (1.0 + np.exp(-z))


def conv(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int, act: int, res: np.ndarray | None = None):
    """x [H, W, Cin], w [Cout, k, k, Cin] (fp16 as stored), b [Cout] -> (y, acc), both float64 [Ho, Wo, Cout]."""
    x = np.asarray(x, np.float64)
    cout, k = w.shape[0], w.shape[1]
    H, W, _ = x.shape
    Ho, Wo = H // stride, W // stride
    cols = im2col(x, k, stride)
    wm = np.asarray(w, np.float64).reshape(cout, -1)
    b = np.asarray(b, np.float64)
    z = cols @ wm.T + b
    acc = np.abs(cols) @ np.abs(wm).T + np.abs(b)
    y = silu(z) if act == 1 else z
    if res is not None:
        r = np.asarray(res, np.float64).reshape(Ho * Wo, cout)
        y = y + r
        acc = acc + np.abs(r)
    return y.reshape(Ho, Wo, cout), acc.reshape(Ho, Wo, cout)


def conv0(x4: np.ndarray, w: np.ndarray, b: np.ndarray):
    """model.0.conv on the engine's 4-channel input [H, W, 4]: channels 0-2 only (3x3 stride 2, SiLU) -> (y, acc)."""
    return conv(np.asarray(x4)[..., :3], w, b, 2, 1)


def dwconv(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int):
    """Depthwise 3x3: x [H, W, C], w [C, 3, 3, 1] (fp16 as stored), b [C] -> (y, acc), float64 [H // stride, W // stride, C].
    Zero padding 1, no activation; acc = |b| + sum |w| |x| as for conv()."""
    x = np.asarray(x, np.float64)
    H, W, Cc = x.shape
    Ho, Wo = H // stride, W // stride
    wd = np.asarray(w, np.float64).reshape(Cc, 3, 3)
    b = np.asarray(b, np.float64)
    xp = np.zeros((H + 2, W + 2, Cc))
    xp[1:1 + H, 1:1 + W] = x
    y = np.broadcast_to(b, (Ho, Wo, Cc)).copy()
    acc = np.broadcast_to(np.abs(b), (Ho, Wo, Cc)).copy()
    for ky in range(3):
        for kx in range(3):
            t = xp[ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            y += t * wd[:, ky, kx]
            acc += np.abs(t) * np.abs(wd[:, ky, kx])
    return y, acc


def _window_max(a: np.ndarray, r: int) -> np.ndarray:
    """Maximum over the clipped (2 r + 1)^2 window around every pixel of a [H, W, C]: separable, rows then columns."""
    H, W = a.shape[:2]
    p = np.full((H + 2 * r, W + 2 * r) + a.shape[2:], -np.inf)
    p[r:r + H, r:r + W] = a
    h = p[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        np.maximum(h, p[:, d:d + W], out=h)
    lo = h[0:H].copy()
    for d in range(1, 2 * r + 1):
        np.maximum(lo, h[d:d + H], out=lo)
    return lo


def sppf(a: np.ndarray):
    """SPPF's pools on a [H, W, C]: (p5, p9, p13), the maxima over the clipped Chebyshev windows of radius 2, 4 and 6
    (= max_pool2d(5, 1, 2) applied once, twice and three times).  Float64; max is exact, so these are a's own values."""
    a = np.asarray(a, np.float64)
    return _window_max(a, 2), _window_max(a, 4), _window_max(a, 6)


def shuffle(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """concat(a, b) + channel shuffle with two groups: out[..., 2 i] = a[..., i], out[..., 2 i + 1] = b[..., i]."""
    assert a.shape == b.shape
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    out[..., 0::2], out[..., 1::2] = a, b
    return out


def op_input(op, tensors: dict) -> np.ndarray:
    """The conv's input, assembled from the slot's tensors (name -> [H, W, C] real values) as the op record says."""
    segs = [op.s0] + ([op.s1] if op.s1.C else [])
    return np.concatenate([segment(np.asarray(tensors[s.tensor.decode()], np.float64), s.coff, s.C, s.shift) for s in segs], axis=-1)


def op_forward(op, tensors: dict, w, b, fuse_wb=None):
    """One conv op of the engine on one slot: (y, acc), or (y, acc, y2, acc2) with y2 the carrier's fused 1x1 (fuse_wb) on y."""
    x = op_input(op, tensors)
    res = None
    if op.res.C:
        res = np.asarray(tensors[op.res.tensor.decode()], np.float64)[..., op.res.coff:op.res.coff + op.cout]
    y, acc = conv(x, w, b, op.stride, op.act, res)
    if fuse_wb is None:
        return y, acc
    w2, b2 = fuse_wb
    y2, acc2 = conv(y, w2, b2, 1, 0)
    return y, acc, y2, acc2
