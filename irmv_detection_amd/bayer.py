"""Host reference of the raw Bayer input format (include/irmv_hip.h, IRMV_SRC_BAYER_*8).

`demosaic` is the exact integer bilinear interpolation the GPU's k_bayer.hip computes; the tests compare the engine with
it bit for bit.  `mosaic` samples an RGB image through a colour filter array to make raw test frames.

The format:
  * a raw frame is uint8 [H][W], H and W even;
  * the pattern names the colours of the 2 x 2 cell at (0,0) (0,1) / (1,0) (1,1);
  * neighbours outside the frame come from reflect-101 indexing (-1 -> 1, W -> W-2), which keeps the CFA phase;
  * a pixel's own colour is its raw value; G at an R or B site is (N + S + E + W + 2) >> 2; B at an R site and R at a
    B site are (NE + NW + SE + SW + 2) >> 2; at a G site the colour of its own row is (W + E + 1) >> 1 and the other
    one (N + S + 1) >> 1;
  * white-balance gains (Q8, 256 = 1.0) apply after the interpolation: min(255, (v * g + 128) >> 8);
  * the output is HWC uint8 with bytes R, G, B.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")


def _red_phase(pattern: str):
    """(row parity, column parity) of the R sites; B sits at the opposite parities."""
    p = pattern.upper()
    if p not in PATTERNS:
        raise ValueError(f"unknown Bayer pattern {pattern!r} (one of {PATTERNS})")
    i = p.index("R")
    return i // 2, i % 2


def mosaic(rgb: np.ndarray, pattern: str) -> np.ndarray:
    """uint8 [H][W][3] RGB -> uint8 [H][W] raw frame: each pixel keeps the one channel its CFA site samples."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be [H][W][3]")
    ry, rx = _red_phase(pattern)
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    ch = np.full((H, W), 1)
    ch[((yy & 1) == ry) & ((xx & 1) == rx)] = 0
    ch[((yy & 1) != ry) & ((xx & 1) != rx)] = 2
    return np.take_along_axis(rgb, ch[..., None], axis=2)[..., 0].astype(np.uint8)


def demosaic(raw: np.ndarray, pattern: str, gains: Sequence[int] = (256, 256, 256)) -> np.ndarray:
    """uint8 [H][W] raw frame -> uint8 [H][W][3] (R, G, B), the engine's demosaic to the bit."""
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.dtype != np.uint8:
        raise ValueError("raw must be a uint8 [H][W] array")
    H, W = raw.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("a Bayer frame has an even width and height")
    g = [int(v) for v in gains]
    if len(g) != 3 or not all(0 <= v <= 1023 for v in g):
        raise ValueError("gains are three Q8 values in [0, 1023]")
    ry, rx = _red_phase(pattern)
    p = np.pad(raw.astype(np.int32), 1, mode="reflect")          # numpy's 'reflect' is reflect-101: -1 -> 1, W -> W-2
    c = p[1:-1, 1:-1]
    n, s, w, e = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    cross = (n + s + w + e + 2) >> 2
    horiz = (w + e + 1) >> 1
    vert = (n + s + 1) >> 1
    yy, xx = np.mgrid[0:H, 0:W]
    r_row = (yy & 1) == ry
    r_col = (xx & 1) == rx
    at_r = r_row & r_col
    at_b = ~r_row & ~r_col
    g_on_r_row = r_row & ~r_col
    g_on_b_row = ~r_row & r_col
    R = np.select([at_r, at_b, g_on_r_row, g_on_b_row], [c, diag, horiz, vert])
    G = np.where(at_r | at_b, cross, c)
    B = np.select([at_b, at_r, g_on_b_row, g_on_r_row], [c, diag, horiz, vert])
    out = np.stack([R, G, B], axis=2)
    gv = np.array(g, np.int32)
    out = np.minimum(255, (out * gv + 128) >> 8)
    return out.astype(np.uint8)
