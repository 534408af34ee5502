"""Host reference of the debug images (irmv_engine_render, csrc/k_render.hip): the node's visualized and binary frames.

`render(R, ...)` computes, bit for bit, the picture the kernel makes from the frame R -- the slot's frame in the coordinates
detections come back in, i.e. `get_rotated_image()` on an engine with rotate180 (include/irmv_hip.h, "debug images"):

  output   ow = W // s, oh = H // s; trailing source columns and rows are dropped
  color    per channel (sum of the s x s block + s*s//2) // (s*s)
  binary   255 on all three channels where any pixel of the block has gray > T,
           gray = (p0*3735 + p1*19235 + p2*9798 + (1 << 14)) >> 15, else 0
  marks    every float truncated toward zero, the window's corner subtracted, floor-divided by s (`coord`).  First the armor
           marks of every record, then per record its box and its label; later marks overwrite earlier ones.
  box      YoloEngine.visualize_bboxes in output coordinates, clamps and all; label: YoloEngine._draw_label with cell 3, 2, 1
  armor    green rings of radius 5, 3, 2 at LB, LT, RT, RB and the segments LT-LB, RT-RB, LT-RT, LB-RB (`ring_mask`,
           `segment_mask`): the project's own rasteriser, not OpenCV's
"""
from __future__ import annotations

import numpy as np

from .engine import ArmorClass, YoloEngine

MARK_BOXES, MARK_LABELS, MARK_ARMORS = 1, 2, 4
MARK_ALL = MARK_BOXES | MARK_LABELS | MARK_ARMORS
CELL = {1: 3, 2: 2, 4: 1}       # glyph cell per scale
RADIUS = {1: 5, 2: 3, 4: 2}     # ring radius per scale
GREEN = (0, 255, 0)
SEGMENTS = ((1, 0), (2, 3), (1, 2), (0, 3))   # indices into LB, LT, RT, RB


def dims(w: int, h: int, scale: int):
    """(ow, oh) of a w x h frame at `scale` (irmv_engine_render_dims)."""
    if scale not in CELL:
        raise ValueError("scale must be 1, 2 or 4")
    return w // scale, h // scale


def coord(v, org: int, scale: int):
    """A mark coordinate in output pixels, or None where the float has none (non-finite, or of magnitude >= 2^24)."""
    v = float(np.float32(v))
    if not np.isfinite(v) or abs(v) >= 2.0 ** 24:
        return None
    return (int(v) - org) // scale


def class_name(class_id: int) -> str:
    return ArmorClass(class_id).name if 0 <= class_id < 14 else "UNKNOWN"


def class_color(class_id: int):
    return (0, 0, 255) if 0 <= class_id <= 6 else (255, 0, 0)


def base(image: np.ndarray, kind: str, scale: int, binary_threshold: int) -> np.ndarray:
    """The picture without marks."""
    s = scale
    ow, oh = dims(image.shape[1], image.shape[0], s)
    blk = image[:oh * s, :ow * s].astype(np.int64).reshape(oh, s, ow, s, 3)
    if kind == "color":
        return ((blk.sum(axis=(1, 3)) + s * s // 2) // (s * s)).astype(np.uint8)
    if kind != "binary":
        raise ValueError("kind must be 'color' or 'binary'")
    gray = (blk[..., 0] * 3735 + blk[..., 1] * 19235 + blk[..., 2] * 9798 + (1 << 14)) >> 15
    bit = (gray > binary_threshold).any(axis=(1, 3))
    return np.repeat((bit * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _window(shape, x0, x1, y0, y1):
    """The part of an oh x ow image inside [x0, x1] x [y0, y1]: (xs, ys) index grids, or None where it is empty."""
    oh, ow = shape
    x0, x1, y0, y1 = max(x0, 0), min(x1, ow - 1), max(y0, 0), min(y1, oh - 1)
    if x0 > x1 or y0 > y1:
        return None
    return np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))


def ring_mask(shape, cx: int, cy: int, r: int) -> np.ndarray:
    """oh x ow bool: the pixels with |dx^2 + dy^2 - r^2| <= 2 r."""
    m = np.zeros(shape, bool)
    g = _window(shape, cx - r - 1, cx + r + 1, cy - r - 1, cy + r + 1)
    if g is not None:
        xs, ys = g
        m[ys, xs] = np.abs((xs - cx) ** 2 + (ys - cy) ** 2 - r * r) <= 2 * r
    return m


def segment_mask(shape, a, b) -> np.ndarray:
    """oh x ow bool: the pixels within distance 1 of the segment a-b, in exact integers.  With d = b - a, L2 = d.d and
    t = (p - a).d:  L2 == 0 or t < 0: |p - a|^2 <= 1;  t > L2: |p - b|^2 <= 1;  else ((p - a) x d)^2 <= L2.
    (Coordinates are below 2^26 in magnitude: every product fits int64 except the last square, which is not formed where
    |(p - a) x d| >= 2^31 -- L2 < 2^54 cannot reach it.)"""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    m = np.zeros(shape, bool)
    g = _window(shape, min(ax, bx) - 1, max(ax, bx) + 1, min(ay, by) - 1, max(ay, by) + 1)   # no other pixel can be that near
    if g is None:
        return m
    xs, ys = g
    dx, dy, qx, qy = bx - ax, by - ay, xs - ax, ys - ay
    L2, t = dx * dx + dy * dy, qx * dx + qy * dy
    ac = np.abs(qx * dy - qy * dx)
    small = ac < 2 ** 31
    line = small & (np.where(small, ac, 0) ** 2 <= L2)
    at_a = qx * qx + qy * qy <= 1
    at_b = (xs - bx) ** 2 + (ys - by) ** 2 <= 1
    m[ys, xs] = np.where((L2 == 0) | (t < 0), at_a, np.where(t > L2, at_b, line))
    return m


def draw_armor(img: np.ndarray, pts, scale: int) -> None:
    """pts: LB, LT, RT, RB as integer (x, y) in output pixels."""
    shape = img.shape[:2]
    m = np.zeros(shape, bool)
    for x, y in pts:
        m |= ring_mask(shape, x, y, RADIUS[scale])
    for i, j in SEGMENTS:
        m |= segment_mask(shape, pts[i], pts[j])
    img[m] = GREEN


def draw_box(img: np.ndarray, x1: int, y1: int, x2: int, y2: int, color) -> None:
    """The rectangle of YoloEngine.visualize_bboxes, with the picture's own size."""
    h, w = img.shape[:2]
    x1c, x2c = max(min(x1, w - 1), 0), max(min(x2, w - 1), 0)
    y1c, y2c = max(min(y1, h - 1), 0), max(min(y2, h - 1), 0)
    for t in range(2):
        for y in (y1 + t, y2 - t):
            if 0 <= y < h:
                img[y, x1c:x2c + 1] = color
        for x in (x1 + t, x2 - t):
            if 0 <= x < w:
                img[y1c:y2c + 1, x] = color


def draw_label(img: np.ndarray, text: str, x: int, y: int, color, cell: int) -> None:
    """YoloEngine._draw_label with a glyph cell of `cell` pixels."""
    h, w = img.shape[:2]
    for k, ch in enumerate(text):
        g = YoloEngine._GLYPHS[ch]
        for r in range(7):
            for c in range(5):
                if (g[r] >> (4 - c)) & 1:
                    x0, y0 = x + k * 6 * cell + c * cell, y - 7 * cell + r * cell
                    img[max(y0, 0):max(min(y0 + cell, h), 0), max(x0, 0):max(min(x0 + cell, w), 0)] = color


def _field(d, name):
    return d[name] if isinstance(d, dict) else getattr(d, name)


def render(image: np.ndarray, kind: str = "color", scale: int = 1, marks: int = MARK_ALL, dets=(), corner=(0, 0),
           binary_threshold: int = 150) -> np.ndarray:
    """The picture of `image` ([H, W, 3] uint8).  dets: records with xyxy, class_id, kpts, armor_valid (capi.Det, or dicts);
    corner: the window's corner for a window slot in the window view, else (0, 0)."""
    img = base(np.asarray(image), kind, scale, binary_threshold)
    org = (int(corner[0]), int(corner[1]))
    recs = []
    for d in dets:
        xy = [coord(v, org[i & 1], scale) for i, v in enumerate(_field(d, "xyxy"))]
        kp = [coord(v, org[i & 1], scale) for i, v in enumerate(_field(d, "kpts"))]
        recs.append((None if None in xy else xy, None if (None in kp or int(_field(d, "armor_valid")) != 1) else kp, int(_field(d, "class_id"))))
    if marks & MARK_ARMORS:
        for _, kp, _ in recs:
            if kp is not None:
                draw_armor(img, [(kp[2 * i], kp[2 * i + 1]) for i in range(4)], scale)
    for xy, _, cls in recs:
        if xy is None:
            continue
        if marks & MARK_BOXES:
            draw_box(img, *xy, class_color(cls))
        if marks & MARK_LABELS:
            draw_label(img, class_name(cls), xy[0], xy[1], class_color(cls), CELL[scale])
    return img
