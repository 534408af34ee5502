"""Host references for rectangular network inputs (net_w x net_h), built from the square oracle's pieces.

The CPU oracle (oracle/) is square-only.  Two restatements extend it, each checked against it where both apply
(tests/test_rect_cpu.py):

  * preprocess(): numpy statement of the integer tap geometry (axis_tap) and the 11-bit bilinear blend of
    preprocess_kernel, per axis.  At W == H it is bit-identical to oracle.preprocess.
  * decode_nms(): a rect head embedded into a square head of side max(W, H) -- rect anchor (level, y, x) -> square
    anchor (level, y, x), every other anchor with class logits of -100 -- run through oracle.decode_nms, anchor indices
    mapped back.  Anchor geometry (x + 0.5) s is the same and the index map is monotone, so the candidate order, ties
    and the survivor order are preserved.

Test infrastructure only; never imported by the product package.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle

RESIZE_STRETCH, RESIZE_LETTERBOX = 0, 1
COEF_BITS = 11
STRIDES = (8, 16, 32)


def letterbox_geom(sw: int, sh: int, W: int, H: int):
    """r = min(W / sw, H / sh); nw = min(W, floor(sw r + 0.5)), nh = min(H, floor(sh r + 0.5)); centred."""
    r = min(W / sw, H / sh)
    nw, nh = min(W, int(np.floor(sw * r + 0.5))), min(H, int(np.floor(sh * r + 0.5)))
    return nw, nh, (W - nw) // 2, (H - nh) // 2


def geometry(sw: int, sh: int, W: int, H: int, mode: int):
    """(nw, nh, px, py) of the resized frame inside the net input."""
    return letterbox_geom(sw, sh, W, H) if mode == RESIZE_LETTERBOX else (W, H, 0, 0)


def axis_taps(dn_total: int, sn: int, dn: int, pad: int, rotate: bool):
    """Per destination coordinate: source pair (i0, i1), weight of i1 in 1/2048, valid flag (False: letterbox pad)."""
    d = np.arange(dn_total, dtype=np.int64)
    r = d - pad
    valid = (r >= 0) & (r < dn)
    num = (2 * r + 1) * sn - dn
    den = 2 * dn
    fl = np.floor_divide(num, den)
    w = (num - fl * den) * 2048 + dn
    w = np.floor_divide(w, den)
    a, b = fl.copy(), fl + 1
    lo, hi = a < 0, a >= sn - 1
    a[lo], b[lo], w[lo] = 0, 0, 0
    a[hi], b[hi], w[hi] = sn - 1, sn - 1, 0
    if rotate:
        a, b = sn - 1 - a, sn - 1 - b
    return np.where(valid, a, 0), np.where(valid, b, 0), np.where(valid, w, 0), valid


def preprocess_u8(src: np.ndarray, W: int, H: int, mode: int = RESIZE_STRETCH, rotate180: bool = True,
                  swap_rb: bool = False) -> np.ndarray:
    """[H][W][3] uint8: the blended pixel values (114 on letterbox padding) the kernels convert to fp16."""
    sh, sw, _ = src.shape
    nw, nh, px, py = geometry(sw, sh, W, H, mode)
    x0, x1, wx, vx = axis_taps(W, sw, nw, px, rotate180)
    y0, y1, wy, vy = axis_taps(H, sh, nh, py, rotate180)
    s = src.astype(np.int64)
    one = 1 << COEF_BITS
    wx_, wy_ = wx[None, :, None], wy[:, None, None]
    top = (one - wx_) * s[y0][:, x0] + wx_ * s[y0][:, x1]
    bot = (one - wx_) * s[y1][:, x0] + wx_ * s[y1][:, x1]
    v = ((one - wy_) * top + wy_ * bot + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS)
    v[~(vy[:, None] & vx[None, :])] = 114
    if swap_rb:
        v = v[..., ::-1]
    return v.astype(np.uint8)


def preprocess(src: np.ndarray, W: int, H: int, mode: int = RESIZE_STRETCH, rotate180: bool = True,
               swap_rb: bool = False) -> np.ndarray:
    """[3][H][W] float32 holding the fp16 values the engine's input tensor holds: half(q / 255.0f)."""
    q = preprocess_u8(src, W, H, mode, rotate180, swap_rb)
    return (q.astype(np.float32) / np.float32(255.0)).astype(np.float16).astype(np.float32).transpose(2, 0, 1).copy()


def num_anchors(W: int, H: int) -> int:
    return sum((H // s) * (W // s) for s in STRIDES)


def anchor_map(W: int, H: int) -> np.ndarray:
    """rect anchor index -> anchor index in the square head of side max(W, H) (monotone increasing)."""
    S = max(W, H)
    out, base = [], 0
    for s in STRIDES:
        h, w, side = H // s, W // s, S // s
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        out.append(base + yy.ravel() * side + xx.ravel())
        base += side * side
    return np.concatenate(out)


def embed_square(head: np.ndarray, W: int, H: int, nc: int) -> np.ndarray:
    S = max(W, H)
    sq = np.zeros((num_anchors(S, S), head.shape[1]), np.float32)
    sq[:, 64:64 + nc] = -100.0
    sq[anchor_map(W, H)] = head
    return sq


def decode_nms(head: np.ndarray, W: int, H: int, nc: int, nk: int, score_thr: float = 0.25, iou_thr: float = 0.45,
               max_det: int = 100, pre_nms_cap: int = 4096) -> dict:
    """oracle.decode_nms of a W x H net's head, through the embedded square head."""
    assert head.shape[0] == num_anchors(W, H)
    S = max(W, H)
    d = oracle.decode_nms(embed_square(head, W, H, nc), S, nc, nk, score_thr, iou_thr, max_det, pre_nms_cap)
    amap = anchor_map(W, H)
    inv = np.full(num_anchors(S, S), -1, np.int64)
    inv[amap] = np.arange(len(amap))
    d["anchors"] = inv[d["anchors"]].astype(np.int32)
    assert (d["anchors"] >= 0).all()
    return d


def anchor_grid(W: int, H: int):
    """Per rect anchor: (x + 0.5, y + 0.5) and stride."""
    cx, cy, st = [], [], []
    for s in STRIDES:
        h, w = H // s, W // s
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        cx.append(xx.ravel() + 0.5)
        cy.append(yy.ravel() + 0.5)
        st.append(np.full(h * w, s))
    return np.concatenate(cx).astype(np.float32), np.concatenate(cy).astype(np.float32), np.concatenate(st).astype(np.float32)


def decode_boxes(head: np.ndarray, W: int, H: int) -> np.ndarray:
    """Direct float64 DFL decode of every anchor's box (xyxy, net pixels): an independent check of the embedding."""
    cx, cy, st = anchor_grid(W, H)
    d = head[:, :64].astype(np.float64).reshape(-1, 4, 16)
    p = np.exp(d - d.max(-1, keepdims=True))
    dist = (p / p.sum(-1, keepdims=True) * np.arange(16)).sum(-1)
    return np.stack([cx - dist[:, 0], cy - dist[:, 1], cx + dist[:, 2], cy + dist[:, 3]], 1) * st[:, None]


def parse_output(boxes: np.ndarray, sw: int, sh: int, W: int, H: int, mode: int) -> np.ndarray:
    """net-input xyxy -> source-frame pixels in float32, per axis: x_src = (x - px) * (sw / nw)."""
    nw, nh, px, py = geometry(sw, sh, W, H, mode)
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    sx, sy = np.float32(sw) / np.float32(nw), np.float32(sh) / np.float32(nh)
    ox, oy = np.float32(px), np.float32(py)
    out = np.empty_like(b)
    out[:, 0::2] = (b[:, 0::2] - ox) * sx
    out[:, 1::2] = (b[:, 1::2] - oy) * sy
    return out
