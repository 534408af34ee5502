"""Plate patches on the host (include/irmv_hip.h, "plate patches"; csrc/k_patch.hip): the reference the kernel is tested
against, in element-wise NumPy.  Every fp64 operation below is one IEEE operation in the order the header writes it (NumPy
fuses nothing), every integer operation is the kernel's; the frame is the one irmv_engine_rotated_image returns.
"""
from __future__ import annotations

import numpy as np

PATCH_W, PATCH_H, PATCH_N = 20, 28, 560
DEFAULTS = dict(span=(32, 54), light_rows=12, top=7)
SPAN_MIN, SPAN_MAX, ROWS_MAX, TOP_MAX = 20, 128, 28, 27


def options(opts=None) -> dict:
    """The options with the defaults filled in; ValueError where the library answers IRMV_ERR_ARG."""
    o = dict(DEFAULTS)
    o.update(opts or {})
    o["span"] = tuple(int(v) for v in o["span"])
    if len(o["span"]) != 2 or any(v < SPAN_MIN or v > SPAN_MAX or (v - PATCH_W) % 2 for v in o["span"]):
        raise ValueError("span must be 20 .. 128 with span - 20 even")
    if not 1 <= o["light_rows"] <= ROWS_MAX:
        raise ValueError("light_rows must be 1 .. 28")
    if not 0 <= o["top"] <= TOP_MAX:
        raise ValueError("top must be 0 .. 27")
    return o


def coefficients(kpts):
    """Heckbert's square-to-quad of the quad kpts (LB, LT, RT, RB; float32 widened) -> (a, b, c, d, e, f, g, h) as float64, or
    None where the record has no patch: a non-finite keypoint, den == 0, a non-finite coefficient."""
    k = np.asarray(kpts, np.float32).reshape(8).astype(np.float64)
    if not np.isfinite(k).all():
        return None
    x0, y0, x1, y1, x2, y2, x3, y3 = k[2], k[3], k[4], k[5], k[6], k[7], k[0], k[1]
    with np.errstate(all="ignore"):
        dx1, dx2, sx = x1 - x2, x3 - x2, ((x0 - x1) + x2) - x3
        dy1, dy2, sy = y1 - y2, y3 - y2, ((y0 - y1) + y2) - y3
        den = dx1 * dy2 - dx2 * dy1
        if den == 0.0:
            return None
        g = (sx * dy2 - dx2 * sy) / den
        h = (dx1 * sy - sx * dy1) / den
        co = np.array([(x1 - x0) + g * x1, (x3 - x0) + h * x3, x0, (y1 - y0) + g * y1, (y3 - y0) + h * y3, y0, g, h], np.float64)
    return co if np.isfinite(co).all() else None


def plate_to_frame(co, s, t):
    """(x, y, w) of plate coordinates (s, t), float64 arrays of one shape."""
    a, b, c, d, e, f, g, h = (np.float64(v) for v in co)
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        w = (g * s + h * t) + 1.0
        x = ((a * s + b * t) + c) / w
        y = ((d * s + e * t) + f) / w
    return x, y, w


def patch_coords(armor_size, o):
    """(s [28, 20], t [28, 20]) of the patch's pixels."""
    span = o["span"][armor_size & 1]
    off = (span - PATCH_W) // 2
    s = (np.arange(PATCH_W, dtype=np.float64) + np.float64(off)) / np.float64(span - 1)
    t = (np.arange(PATCH_H, dtype=np.float64) - np.float64(o["top"])) / np.float64(o["light_rows"])
    return np.broadcast_to(s[None, :], (PATCH_H, PATCH_W)), np.broadcast_to(t[:, None], (PATCH_H, PATCH_W))


def bar_coords(o):
    """(s, t) [2, light_rows + 1]: the two bars' centre lines from their top ends to their bottom ends."""
    n = o["light_rows"] + 1
    t = np.arange(n, dtype=np.float64) / np.float64(o["light_rows"])
    return np.repeat(np.array([0.0, 1.0])[:, None], n, 1), np.broadcast_to(t[None, :], (2, n))


def _guards(x, y, W, H):
    with np.errstate(invalid="ignore"):
        inside = (0.0 <= x) & (x <= W - 1.0) & (0.0 <= y) & (y <= H - 1.0)
        near = (-1.0 <= x) & (x <= float(W)) & (-1.0 <= y) & (y <= float(H))
    return inside, near


def _quantise(v, near):
    q = np.zeros(v.shape, np.int64)
    with np.errstate(all="ignore"):
        q[near] = np.floor(32.0 * v[near] + 0.5).astype(np.int64)
    return q


def texel_gray(frame):
    """The light extraction's gray of every texel, int64 [H, W]."""
    p = frame.astype(np.int64)
    return (p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + (1 << 14)) >> 15


def _fetch(img, ix, iy):
    """img[iy, ix], 0 outside."""
    H, W = img.shape
    ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    out = np.zeros(ix.shape, np.int64)
    out[ok] = img[iy[ok], ix[ok]]
    return out, ok


def otsu(values):
    """(threshold, S) of the integer gray values by the header's integer moments."""
    v = np.asarray(values, np.int64).reshape(-1)
    N, S = int(v.size), int(v.sum())
    hist = np.bincount(v, minlength=256).astype(np.int64)
    w0s, m0s = np.cumsum(hist), np.cumsum(hist * np.arange(256, dtype=np.int64))
    best_q, best_k = -1.0, -1
    for k in range(256):
        w0, m0 = int(w0s[k]), int(m0s[k])
        w1 = N - w0
        if w0 > 0 and w1 > 0:
            A = m0 * N - S * w0
            q = float(np.float64(A * A) / np.float64(w0 * w1))
        else:
            q = -1.0
        if q > best_q:
            best_q, best_k = q, k
    if best_k < 0:      # one gray level: every q is -1
        best_k = int(v[0])
    return best_k, S


def empty(armor_size=0) -> dict:
    return dict(gray=np.zeros((PATCH_H, PATCH_W), np.uint8), state=0, otsu=0, n_outside=0, armor_size=0, bar_sum=(0, 0), sum=0)


def patch(frame, kpts, armor_size, opts=None) -> dict:
    """The record's fields for one quad on `frame` ([H, W, 3] uint8, the rotated image): gray [28, 20] uint8, state, otsu,
    n_outside, armor_size, bar_sum (2), sum."""
    o = options(opts)
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape[:2]
    armor_size = int(armor_size)
    co = coefficients(kpts)
    if co is None:
        return empty()
    s, t = patch_coords(armor_size, o)
    x, y, w = plate_to_frame(co, s, t)
    if not (w > 0.0).all():
        return empty()
    inside, near = _guards(x, y, W, H)
    X, Y = _quantise(x, near), _quantise(y, near)
    ix, fx, iy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    img = texel_gray(frame)
    g00, _ = _fetch(img, ix, iy)
    g10, _ = _fetch(img, ix + 1, iy)
    g01, _ = _fetch(img, ix, iy + 1)
    g11, _ = _fetch(img, ix + 1, iy + 1)
    v = (g00 * (32 - fx) * (32 - fy) + g10 * fx * (32 - fy) + g01 * (32 - fx) * fy + g11 * fx * fy + 512) >> 10
    v[~near] = 0
    thr, S = otsu(v)
    # the bars' colour vote
    bs, bt = bar_coords(o)
    bx, by, _ = plate_to_frame(co, bs, bt)
    _, bnear = _guards(bx, by, W, H)
    BX, BY = (_quantise(bx, bnear) + 16) >> 5, (_quantise(by, bnear) + 16) >> 5
    c0, ok = _fetch(frame[..., 0].astype(np.int64), BX, BY)
    c2, _ = _fetch(frame[..., 2].astype(np.int64), BX, BY)
    take = ok & bnear
    return dict(gray=v.astype(np.uint8), state=1, otsu=thr, n_outside=int((~inside).sum()), armor_size=armor_size,
                bar_sum=(int(c0[take].sum()), int(c2[take].sum())), sum=S)


def rounding_margin(kpts, armor_size, opts, W, H) -> float:
    """The smallest distance of any in-range 32 x + 0.5 or 32 y + 0.5 (the patch's samples and the bars' points) from an
    integer, in quantisation steps: how far every floor() of this quad is from flipping.  inf where the quad has no patch."""
    o = options(opts)
    co = coefficients(kpts)
    if co is None:
        return float("inf")
    m = float("inf")
    for s, t in (patch_coords(int(armor_size), o), bar_coords(o)):
        x, y, w = plate_to_frame(co, s, t)
        _, near = _guards(x, y, W, H)
        for v in (x[near], y[near]):
            if v.size:
                z = 32.0 * v + 0.5
                m = min(m, float(np.abs(z - np.rint(z)).min()))
    return m
