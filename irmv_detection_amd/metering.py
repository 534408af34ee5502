"""Host reference of frame metering (include/irmv_hip.h, "frame metering"; csrc/k_meter.hip).

`meter` is the definition: four 256-bin integer histograms of a rectangle of a slot's frame, in one of two domains.  The GPU
computes the same counts (integer sums do not depend on their order), so the tests compare the engine with it bit for bit,
as they do for bayer.py, render.py and tiles.py.  The helpers below it turn a record into a mean, a percentile, gray-world
white-balance gains and an exposure ratio, in Python ints; the library's irmv_stats_* are the same arithmetic in C.

The rectangle (x0, y0, w, h) is in view-local result coordinates: the frame of the slot's current view as detections see it,
rotated under rotate180; a window slot's corner is not added.  rect=None (w == h == 0) is the whole view; the rectangle is
clipped to the view; an empty intersection gives all-zero histograms, n and rect.

  "view"  `frame` is the view's HWC frame as stored (un-rotated), uint8 [H][W][3].  The samples are the pixels (x, y) of the
          clipped rectangle with (x - rx0) % step == 0 and (y - ry0) % step == 0, (rx0, ry0) the clipped corner.  Rows 0, 1, 2:
          the three channels as stored; row 3: gray = (p0*3735 + p1*19235 + p2*9798 + (1<<14)) >> 15.
  "raw"   `frame` is the raw CFA frame as the producer wrote it, uint8 [FH][FW]; `view_size` is the view's (w, h) and `corner`
          the view's corner inside the raw frame in BUFFER coordinates (window.buffer_origin for a window slot in the window
          view, else (0, 0)).  The clipped rectangle is flipped under rotate180, moved by the corner and shrunk inward to even
          bounds: a grid of 2 x 2 CFA cells.  Cell (i, j), counted from the shrunk region's corner in buffer coordinates, is
          sampled iff i % step == 0 and j % step == 0, and all four of its sites count.  Rows 0, 1, 2: R, G, B sites by
          `pattern` in buffer coordinates; row 3: every sampled site.
"""
from __future__ import annotations

import numpy as np

from . import bayer

DOMAINS = {"view": 0, "raw": 1}
R, G, B, ALL = 0, 1, 2, 3


def geometry(view_size, rect=None, step=1, domain="view", rotate180=True, corner=(0, 0)) -> dict:
    """irmv_meter_map in Python: rect (the record's), region (x, y, w, h in the buffer that is read), phase (view: the first
    sampled column / row of the region), grid (sampled columns, rows -- pixels or cells) and n[4]."""
    if domain not in DOMAINS:
        raise ValueError(f"domain must be one of {sorted(DOMAINS)}, not {domain!r}")
    if step not in (1, 2, 4):
        raise ValueError("step must be 1, 2 or 4")
    vw, vh = int(view_size[0]), int(view_size[1])
    x0, y0, w, h = (0, 0, vw, vh) if rect is None else (int(v) for v in rect)
    if rect is not None and (w < 1 or h < 1):
        raise ValueError("w and h must be at least 1 (rect=None: the whole view)")
    empty = dict(rect=(0, 0, 0, 0), region=(0, 0, 0, 0), phase=(0, 0), grid=(0, 0), n=(0, 0, 0, 0))
    x1, y1 = min(x0 + w, vw), min(y0 + h, vh)
    x0, y0 = max(x0, 0), max(y0, 0)
    if x1 <= x0 or y1 <= y0:
        return empty
    rw, rh = x1 - x0, y1 - y0
    bx, by = (vw - x1, vh - y1) if rotate180 else (x0, y0)
    if domain == "view":
        phase = ((rw - 1) % step, (rh - 1) % step) if rotate180 else (0, 0)
        nx, ny = -(-rw // step), -(-rh // step)
        return dict(rect=(x0, y0, rw, rh), region=(bx, by, rw, rh), phase=phase, grid=(nx, ny), n=(nx * ny,) * 4)
    cx, cy = int(corner[0]), int(corner[1])
    ex0, ex1 = (bx + cx + 1) & ~1, (bx + cx + rw) & ~1
    ey0, ey1 = (by + cy + 1) & ~1, (by + cy + rh) & ~1
    if ex1 <= ex0 or ey1 <= ey0:
        return empty
    bw, bh = ex1 - ex0, ey1 - ey0
    nx, ny = -(-(bw // 2) // step), -(-(bh // 2) // step)
    lx, ly = ex0 - cx, ey0 - cy
    rx, ry = (vw - (lx + bw), vh - (ly + bh)) if rotate180 else (lx, ly)
    s = nx * ny
    return dict(rect=(rx, ry, bw, bh), region=(ex0, ey0, bw, bh), phase=(0, 0), grid=(nx, ny), n=(s, 2 * s, s, 4 * s))


def meter(frame: np.ndarray, rect=None, step=1, domain="view", rotate180=True, pattern=None, view_size=None, corner=(0, 0)) -> dict:
    """The record: hist uint32 [4][256], n uint32 [4], rect (x, y, w, h), domain, step."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8:
        raise ValueError("frame must be uint8")
    if domain == "view":
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("a view frame is [H][W][3]")
        view_size = (frame.shape[1], frame.shape[0])
    else:
        if frame.ndim != 2:
            raise ValueError("a raw frame is [H][W]")
        if pattern is None:
            raise ValueError("the raw domain needs the engine's pattern")
        if view_size is None:
            view_size = (frame.shape[1], frame.shape[0])
    g = geometry(view_size, rect, step, domain, rotate180, corner)
    hist = np.zeros((4, 256), np.int64)
    bx, by, bw, bh = g["region"]
    if g["grid"][0] > 0 and domain == "view":
        px, py = g["phase"]
        s = frame[by + py:by + bh:step, bx + px:bx + bw:step].astype(np.int64).reshape(-1, 3)
        gray = (s[:, 0] * 3735 + s[:, 1] * 19235 + s[:, 2] * 9798 + (1 << 14)) >> 15
        for r, v in enumerate((s[:, 0], s[:, 1], s[:, 2], gray)):
            hist[r] = np.bincount(v, minlength=256)
    elif g["grid"][0] > 0:
        ry, rx = bayer._red_phase(pattern)
        yy, xx = np.mgrid[by:by + bh, bx:bx + bw]
        sampled = (((yy - by) // 2) % step == 0) & (((xx - bx) // 2) % step == 0)
        at_r = ((yy & 1) == ry) & ((xx & 1) == rx)
        at_b = ((yy & 1) != ry) & ((xx & 1) != rx)
        v = frame[by:by + bh, bx:bx + bw]
        for r, m in enumerate((at_r, ~at_r & ~at_b, at_b, np.ones_like(at_r))):
            hist[r] = np.bincount(v[m & sampled], minlength=256)
    n = hist.sum(axis=1)
    assert tuple(int(v) for v in n) == tuple(g["n"])
    return dict(hist=hist.astype(np.uint32), n=n.astype(np.uint32), rect=tuple(g["rect"]), domain=DOMAINS[domain], step=int(step))


# ---- what a record says: Python ints throughout -----------------------------------------------------------------------------
def _row(stats, row):
    if not 0 <= row <= 3:
        raise ValueError("row must be 0..3")
    return [int(v) for v in np.asarray(stats["hist"])[row]]


def _sums(h, lo, hi):
    if not (0 <= lo <= 255 and 0 <= hi <= 255):
        raise ValueError("lo and hi must be 0..255")
    return sum(v * h[v] for v in range(lo, hi + 1)), sum(h[v] for v in range(lo, hi + 1))


def mean_q8(stats, row, lo=0, hi=255):
    """((256 S + N // 2) // N, N) with S = sum v h[v], N = sum h[v] over lo <= v <= hi; (0, 0) where N == 0."""
    S, N = _sums(_row(stats, row), lo, hi)
    return ((256 * S + N // 2) // N, N) if N else (0, 0)


def percentile(stats, row, num, den):
    """The smallest v with cum(v) * den >= num * n[row]."""
    h = _row(stats, row)
    n = int(np.asarray(stats["n"])[row])
    if den <= 0 or not 0 <= num <= den:
        raise ValueError("the percentile needs den > 0 and 0 <= num <= den")
    if n == 0:
        raise ValueError("the row has no sample")
    cum = 0
    for v in range(256):
        cum += h[v]
        if cum * den >= num * n:
            return v
    return 255


def gray_world(stats, lo=8, hi=247):
    """Q8 gains (R, 256, B) that bring the R and B means over [lo, hi] to the G mean, each at most 1023.  Raw records only;
    ValueError where a channel has no mass in the range."""
    if int(stats["domain"]) != DOMAINS["raw"]:
        raise ValueError("gray_world reads a raw record")
    S, N = zip(*(_sums(_row(stats, c), lo, hi) for c in (R, G, B)))
    out = [0, 256, 0]
    for c in (R, B):
        d = S[c] * N[G]
        if d == 0:
            raise ValueError("no R, G or B mass inside [lo, hi]")
        out[c] = min(1023, (256 * S[G] * N[c] + d // 2) // d)
    return tuple(out)


def exposure_q8(stats, row, num, den, target):
    """clamp((256 target + p // 2) // max(p, 1), 16, 4096), p that percentile: the factor (Q8) for the exposure time."""
    if not 0 <= target <= 255:
        raise ValueError("target must be 0..255")
    p = percentile(stats, row, num, den)
    return min(max((256 * target + p // 2) // max(p, 1), 16), 4096)
