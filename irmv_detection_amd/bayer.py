"""Host reference of the raw Bayer input format (include/irmv_hip.h, IRMV_SRC_BAYER_*8).

`demosaic` is the exact integer arithmetic the GPU's k_bayer.hip computes, for both interpolations; the tests compare the
engine with it bit for bit.  `mosaic` samples an RGB image through a colour filter array to make raw test frames.

The format:
  * a raw frame is uint8 [H][W], H and W even;
  * the pattern names the colours of the 2 x 2 cell at (0,0) (0,1) / (1,0) (1,1);
  * neighbours outside the frame come from reflect-101 indexing (-1 -> 1, W -> W-2), which keeps the CFA phase;
  * a pixel's own colour is its raw value; G at an R or B site is (N + S + E + W + 2) >> 2; B at an R site and R at a
    B site are (NE + NW + SE + SW + 2) >> 2; at a G site the colour of its own row is (W + E + 1) >> 1 and the other
    one (N + S + 1) >> 1;
  * algo="mhc" (IRMV_DEMOSAIC_MHC): the 5 x 5 Malvar-He-Cutler filters instead.  Reflect-101 at radius 2 (-2 -> 2,
    W + 1 -> W - 3; H, W >= 4); a pixel's own colour is its raw value; the others are clamp((s + 8) >> 4, 0, 255) of a signed
    sum in sixteenths (floor shift), with C the centre, S1 / S2 the four axis neighbours at distance 1 / 2, X the diagonals:
    G at R or B: 8 C + 4 S1 - 2 S2; at a G site the colour sampled in its row: 10 C + 8 (W1 + E1) - 2 X - 2 (W2 + E2) +
    (N2 + S2), the one sampled in its column: the same with the axes swapped; B at R and R at B: 12 C + 4 X - 3 S2;
  * white-balance gains (Q8, 256 = 1.0) apply after the interpolation: min(255, (v * g + 128) >> 8), then an optional
    per-channel tone LUT: out = lut[c][that] -- together one table `isp_table(gains, lut)[c][v]`, which is what the engine
    keeps in device memory (irmv_engine_set_bayer_isp);
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


def _gains(gains):
    g = [int(v) for v in gains]
    if len(g) != 3 or not all(0 <= v <= 1023 for v in g):
        raise ValueError("gains are three Q8 values in [0, 1023]")
    return g


def isp_table(gains: Sequence[int] = (256, 256, 256), lut=None) -> np.ndarray:
    """uint8 [3][256]: T[c][v] = lut[c][min(255, (v * gains[c] + 128) >> 8)], the gains and the tone LUT (uint8 [256] or
    [3][256], None = identity) as the one table the engine folds them into."""
    g = np.array(_gains(gains), np.int64)
    v = np.arange(256, dtype=np.int64)
    t = np.minimum(255, (v[None, :] * g[:, None] + 128) >> 8)
    if lut is None:
        return t.astype(np.uint8)
    lut = np.asarray(lut)
    if lut.dtype != np.uint8 or lut.shape not in ((256,), (3, 256)):
        raise ValueError("lut must be a uint8 [256] or [3][256] array")
    lut = np.broadcast_to(lut, (3, 256))
    return np.take_along_axis(lut, t, axis=1).astype(np.uint8)


def _mhc(raw, r_row, r_col):
    """int32 [H][W][3] before the table: the Malvar-He-Cutler sums, rounded and clamped."""
    H, W = raw.shape
    p = np.pad(raw.astype(np.int32), 2, mode="reflect")          # -1 -> 1, -2 -> 2, W -> W-2, W+1 -> W-3

    def at(dy, dx):
        return p[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    c = at(0, 0)
    ns1, we1 = at(-1, 0) + at(1, 0), at(0, -1) + at(0, 1)
    ns2, we2 = at(-2, 0) + at(2, 0), at(0, -2) + at(0, 2)
    x4 = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)

    def fin(s):
        return np.clip((s + 8) >> 4, 0, 255)
    g_at_rb = fin(8 * c + 4 * (ns1 + we1) - 2 * (ns2 + we2))
    opposite = fin(12 * c + 4 * x4 - 3 * (ns2 + we2))
    in_row = fin(10 * c + 8 * we1 - 2 * x4 - 2 * we2 + ns2)
    in_col = fin(10 * c + 8 * ns1 - 2 * x4 - 2 * ns2 + we2)
    at_r, at_b = r_row & r_col, ~r_row & ~r_col
    g_on_r_row, g_on_b_row = r_row & ~r_col, ~r_row & r_col
    R = np.select([at_r, at_b, g_on_r_row, g_on_b_row], [c, opposite, in_row, in_col])
    G = np.where(at_r | at_b, g_at_rb, c)
    B = np.select([at_b, at_r, g_on_b_row, g_on_r_row], [c, opposite, in_row, in_col])
    return np.stack([R, G, B], axis=2)


def demosaic(raw: np.ndarray, pattern: str, gains: Sequence[int] = (256, 256, 256), algo: str = "bilinear", lut=None) -> np.ndarray:
    """uint8 [H][W] raw frame -> uint8 [H][W][3] (R, G, B), the engine's demosaic to the bit.  algo: "bilinear" or "mhc";
    lut: the tone LUT behind the gains (isp_table)."""
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.dtype != np.uint8:
        raise ValueError("raw must be a uint8 [H][W] array")
    H, W = raw.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("a Bayer frame has an even width and height")
    g = _gains(gains)
    if algo not in ("bilinear", "mhc"):
        raise ValueError(f"unknown demosaic algorithm {algo!r} (\"bilinear\" or \"mhc\")")
    ry, rx = _red_phase(pattern)
    if algo == "mhc":
        if H < 4 or W < 4:
            raise ValueError("the MHC demosaic needs a frame of at least 4 x 4")
        yy, xx = np.mgrid[0:H, 0:W]
        out = _mhc(raw, (yy & 1) == ry, (xx & 1) == rx)
        return isp_table(g, lut)[np.arange(3), out]
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
    if lut is not None:
        out = isp_table((256, 256, 256), lut)[np.arange(3), out]
    return out.astype(np.uint8)
