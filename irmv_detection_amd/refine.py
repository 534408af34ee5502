"""Host reference of the refined point source (IRMV_POINTS_REFINED, include/irmv_hip.h; k_light.hip's guided instantiation).

Bit-exact restatement of the rules that do not need an image: usable keypoints (rule 1), the guided ROI's box (rule 2), the
cost, admission and choice of a light per side (rules 4 and 5) and the flag (rule 8).  Everything is numpy float32 in the
association order the kernel is written in (it is compiled without contraction).  The lights themselves (rule 3) are the
classical extraction's; a caller composes them from whatever extraction it trusts and hands them to `select`.
"""
from __future__ import annotations

import numpy as np

DEFAULT_SNAP = 0.5          # irmv_engine_set_refine's defaults; neither has been validated on a trained model
DEFAULT_ROI_MARGIN = 4.0    # source pixels
SNAP_RANGE = (0.0, 4.0)     # (0, 4]
ROI_MARGIN_RANGE = (0.0, 64.0)   # [0, 64]
PIXEL_LIMIT = 16777216.0    # 2^24: pnp_device.hpp pixel_in_range

REFINED, KEPT, NO_ANSWER = 1, 0, -1   # the flag (irmv_det.reserved)

_f = np.float32


def check_params(snap, roi_margin) -> None:
    """The setter's validation: snap in (0, 4], roi_margin in [0, 64]; NaN fails both."""
    s, m = _f(snap), _f(roi_margin)
    if not (s > _f(0) and s <= _f(4)):
        raise ValueError("snap must be in (0, 4]")
    if not (m >= _f(0) and m <= _f(64)):
        raise ValueError("roi_margin must be in [0, 64]")


def usable(kpts) -> bool:
    """Rule 1: all eight values finite and below 2^24 in magnitude."""
    k = np.asarray(kpts, np.float32).reshape(8)
    return bool(np.all(np.abs(k) < _f(PIXEL_LIMIT)))      # (NaN compares false)


def _min(a, b):
    return a if a < b else b


def _max(a, b):
    return a if a > b else b


def guided_box(xyxy, kpts, margin):
    """Rule 2: -> float32 [4] (gx1, gy1, gx2, gy2), the box that goes through the classical ROI rule (clamp to the frame,
    truncate), or None where the keypoints are unusable (rule 1: no extraction, nothing of the label pool).
    min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b, the keypoints folded first, in order."""
    if not usable(kpts):
        return None
    b = np.asarray(xyxy, np.float32).reshape(4)
    k = np.asarray(kpts, np.float32).reshape(4, 2)
    m = _f(margin)
    nx, ny, mx, my = k[0, 0], k[0, 1], k[0, 0], k[0, 1]
    for i in range(1, 4):
        nx, mx = _min(k[i, 0], nx), _max(k[i, 0], mx)
        ny, my = _min(k[i, 1], ny), _max(k[i, 1], my)
    return np.array([_min(b[0], nx) - m, _min(b[1], ny) - m, _max(b[2], mx) + m, _max(b[3], my) + m], np.float32)


def _d2(p, q):
    dx, dy = _f(p[0]) - _f(q[0]), _f(p[1]) - _f(q[1])
    return _f(_f(dx * dx) + _f(dy * dy))


def cost(bottom, top, B, T):
    """Rule 4: ((b.x-B.x)^2 + (b.y-B.y)^2) + ((t.x-T.x)^2 + (t.y-T.y)^2), float32."""
    return _f(_d2(bottom, B) + _d2(top, T))


def sides(kpts):
    """-> ((B, T) of side L, (B, T) of side R): L = (kpts[0..1], kpts[2..3]), R = (kpts[6..7], kpts[4..5])."""
    k = np.asarray(kpts, np.float32).reshape(4, 2)
    return (k[0], k[1]), (k[3], k[2])


def select(lights, kpts, snap):
    """Rules 4 to 6 without PnP.  lights: [(contour index, bottom (x, y), top (x, y))] of the ROI's gated lights, in any
    order; kpts: the eight prior values.  -> (refined, iL, iR): the contour indices chosen for the sides (None: no admissible
    light), refined = both exist and differ.  Per side the admissible light (cost <= (snap * snap) * len2) of least cost, on
    equal cost the higher contour index."""
    if not usable(kpts):
        return False, None, None
    s = _f(snap)
    s2 = _f(s * s)
    pick = []
    for B, T in sides(kpts):
        thr = _f(s2 * _d2(B, T))
        best = None                          # (cost, index)
        for idx, b, t in lights:
            c = cost(b, t, B, T)
            if not c <= thr:
                continue
            if best is None or c < best[0] or (c == best[0] and idx > best[1]):
                best = (c, idx)
        pick.append(None if best is None else best[1])
    iL, iR = pick
    return (iL is not None and iR is not None and iL != iR), iL, iR


def flag(no_answer: bool, refined: bool, pnp_ok: bool = True) -> int:
    """Rule 8: -1 where the extraction had no answer (pool, contour or point limit), 1 where a pair was chosen and PnP
    accepted its quad, else 0."""
    if no_answer:
        return NO_ANSWER
    return REFINED if (refined and pnp_ok) else KEPT


def label_bytes(rw: int, rh: int) -> int:
    """Bytes of the label pool a ROI of rw x rh takes: its zero-bordered label image, rounded up to 16."""
    return ((rw + 2) * (rh + 2) + 15) & ~15
