"""A seeded zoo of source geometries for the input stage (k_pre.hip, k_bayer.hip, k_front.hip and the host geometry of
engine.cpp that drives them), an independent float64 reference of the resize, and an independent model of the front's plan.

An Entry is one engine configuration: source (W, H), net (w, h), resize mode, rotate180, swap_rb, source format (HWC, or
a Bayer pattern with gains), slot count, and the labels of the categories it stands for.  `ZOO` is the whole list;
tests/test_input_geometry.py asserts the category counts (MINIMUM) on the CPU and tests/test_gpu_input_geometry.py runs
every entry on the GPU.

Net sizes are the smallest that still reach every path of the front kernel, whose path depends on ratios and residues and
not on the absolute net size: 64, 96, 128, 160 and 256, square and 64 x 96, 96 x 64, 128 x 64, 256 x 64 (w x h).  A net
width that is no multiple of 64 gives a partial last tile column (W1 = net_w / 4 is no multiple of 16).  The net height
is a multiple of 32, so H1 = net_h / 4 is always a multiple of 8: there are NO partial tile rows, on the 4-row tile or on
the 8-row tile -- do not look for them.

The reference (`reference`) is a float64 half-pixel-centre bilinear resize with the letterbox box and the rotation
written out in numpy: rotate the source, resize it into the box, grey elsewhere.  It shares no code with the oracle's C
or with the engine.  `reference(..., variant=...)` gives the classic wrong variants the tests must be able to see.  Bayer
entries are demosaiced first with irmv_detection_amd.bayer.demosaic; `demosaic_border` restates it with a border rule as a
parameter, for the two wrong border variants.

`expected_plan` is a numpy model of what irmv_front_plan must report, from the tap tables of tests/rect_ref.py.

Test infrastructure only; never imported by the product package."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import rect_ref
from irmv_detection_amd import bayer, frames

STRETCH, LETTERBOX = 0, 1
BAND = 8                      # kBayerBandRows (irmv_common.hpp)
TILE_X, TILE_Y, TILE_Y_DIRECT = 16, 4, 8
STAGE_MAX = 128 * 1024        # kFrontStageMax
FUSED, MOD4, TAP_RANGE, STAGE_LIMIT = "fused", "sw % 4", "pitch or rows over 1023", "region over the stage limit"
ID_GAINS, SAT_GAINS = (256, 256, 256), (600, 200, 1023)
SEED = 20261018


@dataclass(frozen=True)
class Entry:
    name: str
    cats: tuple            # category labels (MINIMUM's keys)
    src: tuple             # (W, H)
    net: tuple             # (w, h)
    mode: int = STRETCH
    rot: bool = True
    swap: bool = False
    fmt: str = "HWC"       # or a Bayer pattern
    gains: tuple = ID_GAINS
    slots: int = 1
    expect: str = FUSED    # FUSED, or the reason the plan must state
    direct: bool = False   # exact 2 : 1 columns: direct tiles (and the 8-row tile where fused)

    @property
    def frame_bytes(self):
        return self.src[0] * self.src[1] * 3

    @property
    def src_bytes(self):
        return self.src[0] * self.src[1] * (3 if self.fmt == "HWC" else 1)


# ---- the float64 reference -------------------------------------------------------------------------------------------
def letterbox(sw, sh, W, H, mode, pad_up=False):
    """(nw, nh, px, py): include/irmv_hip.h's statement of the box."""
    if mode != LETTERBOX:
        return W, H, 0, 0
    r = min(W / sw, H / sh)
    nw, nh = min(W, int(np.floor(sw * r + 0.5))), min(H, int(np.floor(sh * r + 0.5)))
    half = (lambda v: (v + 1) // 2) if pad_up else (lambda v: v // 2)
    return nw, nh, half(W - nw), half(H - nh)


def _axis(sn, dn, variant):
    """Source pair and weight of destination samples 0 .. dn - 1 of an axis of sn source samples."""
    d = np.arange(dn, dtype=np.float64)
    f = d * (sn - 1) / max(dn - 1, 1) if variant == "corner_aligned" else (d + 0.5) * sn / dn - 0.5
    f = np.clip(f, 0.0, sn - 1.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), sn - 1)
    i1 = np.minimum(i0 + 1, max(sn - 2, 0) if variant == "clamp_early" else sn - 1)
    return i0, i1, f - i0


def reference(frame, net, mode=STRETCH, rot=True, swap=False, variant=None):
    """float64 [h][w][3] in 0 .. 255: what the net input holds before /255, 114 on the padding."""
    W, H = net
    src = np.asarray(frame, np.float64)
    late = variant == "rotate_after_pad"
    if rot and not late:
        src = src[::-1, ::-1]
    if swap:
        src = src[..., ::-1]
    sh, sw, _ = src.shape
    nw, nh, px, py = letterbox(sw, sh, W, H, mode, pad_up=variant == "pad_round_up")
    out = np.full((H, W, 3), 114.0)
    if nw > 0 and nh > 0:
        x0, x1, wx = _axis(sw, nw, variant)
        y0, y1, wy = _axis(sh, nh, variant)
        wx_, wy_ = wx[None, :, None], wy[:, None, None]
        top = src[y0][:, x0] * (1 - wx_) + src[y0][:, x1] * wx_
        bot = src[y1][:, x0] * (1 - wx_) + src[y1][:, x1] * wx_
        out[py:py + nh, px:px + nw] = top * (1 - wy_) + bot * wy_
    return out[::-1, ::-1] if (rot and late) else out


VARIANTS = ("clamp_early", "corner_aligned", "rotate_after_pad", "pad_round_up")


def demosaic_border(raw, pattern, gains=ID_GAINS, border="reflect101"):
    """bayer.demosaic with the border rule as a parameter.  reflect101: -1 -> 1, N -> N - 2 (the format; keeps the CFA
    phase).  reflect: -1 -> 0, N -> N - 1 (the neighbour is a site of another colour).  far_clamp: reflect-101 at the near
    border, N -> N - 1 at the far one (the phase is lost at the right and bottom border only)."""
    raw = np.asarray(raw)
    H, W = raw.shape

    def idx(n):
        i = np.arange(-1, n + 1)
        lo = {"reflect101": 1, "reflect": 0, "far_clamp": 1}[border]
        hi = {"reflect101": n - 2, "reflect": n - 1, "far_clamp": n - 1}[border]
        return np.where(i < 0, lo, np.where(i >= n, hi, i))
    p = raw.astype(np.int64)[idx(H)][:, idx(W)]
    c = p[1:-1, 1:-1]
    n, s, w, e = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    cross, horiz, vert = (n + s + w + e + 2) >> 2, (w + e + 1) >> 1, (n + s + 1) >> 1
    k = pattern.index("R")
    yy, xx = np.mgrid[0:H, 0:W]
    r_row, r_col = (yy & 1) == k // 2, (xx & 1) == k % 2
    R = np.where(r_row, np.where(r_col, c, horiz), np.where(r_col, vert, diag))
    G = np.where(r_row == r_col, cross, c)
    B = np.where(r_row, np.where(r_col, diag, vert), np.where(r_col, horiz, c))
    out = np.stack([R, G, B], axis=2)
    return np.minimum(255, (out * np.array(gains, np.int64) + 128) >> 8).astype(np.uint8)


# ---- frames ----------------------------------------------------------------------------------------------------------
def slot_frames(e: Entry, seed=0):
    """One distinct frame per slot: uniform random bytes, the upper half a frames.synthetic_frame.  -> (what goes into the
    slot, the HWC frame every later stage sees); the two are the same array for an HWC entry."""
    W, H = e.src
    out = []
    for s in range(e.slots):
        rng = np.random.default_rng([SEED, seed, s, W, H])
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[: H // 2] = frames.synthetic_frame(17 + 3 * s + seed, W, H)[: H // 2]
        if e.fmt == "HWC":
            out.append((img, img))
        else:
            raw = bayer.mosaic(img, e.fmt)
            if e.gains != ID_GAINS:
                raw = np.maximum(raw, rng.integers(0, 256, raw.shape, dtype=np.uint8))   # bright enough to saturate
            out.append((raw, bayer.demosaic(raw, e.fmt, e.gains)))
    return out


# ---- a model of the plan ---------------------------------------------------------------------------------------------
def tile_classes(box, net, tile_y):
    """(inside, x_edge, y_edge, corner): a tile of model.1's output (tile_y x 16) reads net-input columns
    [64 i - 3, 64 i + 64) and rows [4 tile_y j - 3, 4 tile_y (j + 1)); it is inside on an axis when all of them have a source."""
    W, H = net
    nx, ny = -(-(W // 4) // TILE_X), -(-(H // 4) // tile_y)
    in_x = [4 * TILE_X * i - 3 >= box[0] and 4 * TILE_X * (i + 1) <= min(box[1], W) for i in range(nx)]
    in_y = [4 * tile_y * j - 3 >= box[2] and 4 * tile_y * (j + 1) <= min(box[3], H) for j in range(ny)]
    ax, ay = sum(in_x), sum(in_y)
    return ax * ay, (nx - ax) * ay, ax * (ny - ay), (nx - ax) * (ny - ay)


def expected_plan(e: Entry):
    """What irmv_front_plan must report for e, from the tap tables of tests/rect_ref.py."""
    (sw, sh), (W, H) = e.src, e.net
    nw, nh, px, py = letterbox(sw, sh, W, H, e.mode)
    box = (px, px + nw, py, py + nh)
    x0, x1, _, vx = rect_ref.axis_taps(W, sw, nw, px, e.rot)
    y0, y1, _, vy = rect_ref.axis_taps(H, sh, nh, py, e.rot)

    def spans(a, b, valid, n, tile):
        out = []
        for t in range(-(-(n // 4) // tile)):
            g = np.arange(4 * t * tile - 3, 4 * (t + 1) * tile)
            g = g[(g >= 0) & (g < n)]
            g = g[valid[g]]
            if len(g):
                out.append((int(min(a[g].min(), b[g].min())), int(max(a[g].max(), b[g].max()))))
        return out
    pitch = max([min((hi + 4) & ~3, sw) - (lo & ~3) for lo, hi in spans(x0, x1, vx, W, TILE_X)], default=0)
    rows = max([hi - lo + 1 for lo, hi in spans(y0, y1, vy, H, TILE_Y)], default=0)
    if sw % 4:
        reason = MOD4
    elif pitch > 1023 or rows > 1023:
        reason = TAP_RANGE
    elif pitch * rows * 4 > STAGE_MAX:
        reason = STAGE_LIMIT
    else:
        reason = FUSED
    direct = nw > 0 and sw == 2 * nw              # every column tap is the pair (2 k, 2 k + 1) at 1/2 : 1/2
    tile_y = TILE_Y_DIRECT if direct and reason == FUSED else TILE_Y
    cases = set()
    if direct:
        step, m0 = (-2, sw - 2) if e.rot else (2, 0)
        for i in range(-(-(W // 4) // TILE_X)):
            mq = m0 + step * (4 * TILE_X * i - 3 - px)
            cases.add(("+" if step > 0 else "-", mq % 4))
    return dict(reason=reason, fused=reason == FUSED, direct=direct, tile_y=tile_y, box=box, classes=tile_classes(box, (W, H), tile_y),
                pair_cases=cases, fx_i0=((sw - 2) if e.rot else 0) if direct else 0, fx_step=-2 if e.rot else 2,
                upload_kernel=e.src_bytes % 16 == 0, tiles=(-(-(W // 4) // TILE_X), -(-(H // 4) // tile_y)))


PAIR_BITS = {("+", 0): 1, ("+", 2): 2, ("-", 0): 4, ("-", 2): 8}


# ---- the zoo ---------------------------------------------------------------------------------------------------------
def _slots(src, fmt="HWC"):
    """3 slots wherever slots 1 and 2 would start misaligned (frame bytes or raw bytes no multiple of 16)."""
    W, H = src
    return 3 if (W * H * 3) % 16 or (W * H) % 16 or fmt != "HWC" else 1


def _e(name, cats, src, net, mode=STRETCH, rot=True, swap=False, expect=FUSED, direct=False, slots=None, fmt="HWC", gains=ID_GAINS):
    net = (net, net) if isinstance(net, int) else net
    cats = tuple(cats) + (f"sw%4={src[0] % 4}", "sw%16=0" if src[0] % 16 == 0 else "sw%16!=0", f"slots={slots or _slots(src, fmt)}")
    return Entry(name, cats, tuple(src), net, mode, rot, swap, fmt, gains, slots or _slots(src, fmt), expect, direct)


def build_zoo():
    Z = []
    # ---- ratio per axis
    Z += [_e("identity 64", ["identity"], (64, 64), 64, rot=False),
          _e("identity 96x64 rot", ["identity"], (96, 64), (96, 64)),
          _e("identity 128 3 slots", ["identity"], (128, 128), 128, swap=True, slots=3)]
    Z += [_e("2:1 64", ["2:1"], (128, 128), 64, rot=False, direct=True),                         # (+, 2)
          _e("2:1 128 rot 3 slots", ["2:1", "2:1 rot"], (256, 256), 128, direct=True, slots=3),   # (-, 0); inside, y-edge and corner direct tiles
          _e("2:1 160 partial column", ["2:1"], (320, 320), 160, rot=False, swap=True, direct=True),
          _e("2:1 256x64 rot", ["2:1", "2:1 rot"], (512, 128), (256, 64), direct=True),
          _e("2:1 one pad column each side", ["2:1", "pad x", "pad even", "pad one column"], (124, 128), 64, LETTERBOX, rot=False, direct=True),        # (+, 0)
          _e("2:1 one pad column each side rot", ["2:1", "2:1 rot", "pad x", "pad even", "pad one column"], (252, 256), 128, LETTERBOX, direct=True),   # (-, 2)
          _e("2:1 even pad rot", ["2:1", "2:1 rot", "pad x", "pad even"], (248, 256), 128, LETTERBOX, direct=True, slots=3),
          _e("2:1 columns, rows on .5", ["2:1", "pad y", "round .5"], (128, 65), 64, LETTERBOX, rot=False, direct=True),
          _e("2:1 box of 4 columns", ["2:1", "2:1 rot", "pad x", "narrow box"], (8, 128), 64, LETTERBOX, direct=True),
          _e("2:1 128x64 box of 6 rows rot", ["2:1", "2:1 rot", "pad y", "narrow box"], (256, 12), (128, 64), LETTERBOX, direct=True)]
    Z += [_e("3:1 64", ["3:1"], (192, 192), 64), _e("3:1 128", ["3:1"], (384, 384), 128, rot=False, slots=3),
          _e("4:1 64", ["4:1"], (256, 256), 64, rot=False), _e("4:1 128x64", ["4:1"], (512, 256), (128, 64), swap=True)]
    Z += [_e("7:1 over the stage", ["stage limit"], (448, 448), 64, expect=STAGE_LIMIT),
          _e("6:1 128 over the stage", ["stage limit"], (768, 768), 128, rot=False, expect=STAGE_LIMIT),
          _e("20:1 pitch over 1023", ["tap range"], (1280, 64), 64, expect=TAP_RANGE),
          _e("66:1 rows over 1023", ["tap range", "tall source"], (64, 4224), 64, rot=False, expect=TAP_RANGE),
          _e("widest source", ["tap range", "sw=4096"], (4096, 64), 64, expect=TAP_RANGE),
          _e("widest source less one", ["sw=4095"], (4095, 64), 64, rot=False, expect=MOD4, slots=3)]
    Z += [_e("up 2x2", ["strong up", "src 2"], (2, 2), 64, expect=MOD4),
          _e("up 2x1200", ["strong up", "src 2"], (2, 1200), 64, rot=False, expect=MOD4),
          _e("up 4096x2", ["strong up", "src 2", "sw=4096"], (4096, 2), 64, expect=TAP_RANGE),
          _e("up 3x3", ["strong up", "src 3"], (3, 3), 64, expect=MOD4),
          _e("up 4x4", ["strong up", "src 4"], (4, 4), 64),
          _e("up 4x4 128 rot", ["strong up", "src 4"], (4, 4), 128, swap=True, slots=3),
          _e("up 5x5", ["strong up", "src 5"], (5, 5), (96, 64), expect=MOD4),
          _e("up 8x8", ["strong up", "src 8"], (8, 8), 128, rot=False),
          _e("up 16x16", ["strong up", "src 16"], (16, 16), 160),
          _e("up 16x3 letterbox", ["strong up", "src 16", "src 3", "pad y"], (16, 3), 128, LETTERBOX, rot=False),
          _e("up 4x1200 thin", ["strong up", "src 4"], (4, 1200), 64),
          _e("up 800x4 flat", ["strong up", "src 4"], (800, 4), (128, 64), rot=False)]
    # ---- letterbox
    Z += [_e("pad x odd", ["pad x", "pad odd"], (100, 170), 128, LETTERBOX),              # nw = 75: 26 columns left, 27 right
          _e("pad y even", ["pad y", "pad even"], (200, 125), 128, LETTERBOX, rot=False),  # nh = 80: 24 rows above and below
          _e("pad y odd total rot", ["pad y", "pad odd"], (200, 120), 128, LETTERBOX),     # nh = 77: 25 rows above, 26 below
          _e("one pad column on the right", ["pad x", "pad one column"], (252, 256), (64, 64), LETTERBOX, rot=False),   # nw = 63
          _e("one pad row below rot", ["pad y", "pad one row"], (256, 252), 64, LETTERBOX),
          _e("one pad row each side", ["pad y", "pad one row", "pad even"], (128, 126), 128, LETTERBOX, rot=False),
          _e("rounding on .5", ["round .5", "pad y", "2:1", "2:1 rot"], (256, 129), 128, LETTERBOX, direct=True),   # nh = 64.5 -> 65; columns at 2 : 1
          _e("box narrower than a tile", ["narrow box", "pad x"], (12, 200), 128, LETTERBOX, rot=False),
          _e("box lower than a tile 256x64", ["narrow box", "pad y"], (1000, 20), (256, 64), LETTERBOX)]
    # ---- seeded: non-integer down-scales and mild up-scales, one per width residue
    rng = np.random.default_rng(SEED)
    nets = [(64, 64), (96, 96), (128, 128), (160, 160), (256, 256), (64, 96), (96, 64), (128, 64), (256, 64)]
    k = 0
    for cat, lo, hi in (("down", 1.05, 4.4), ("mild up", 0.6, 0.98)):
        for res in range(4):                        # every sw % 4
            W, H = nets[k % len(nets)]
            k += 1
            sw = int(round(W * rng.uniform(lo, hi))) // 4 * 4 + res
            sh = min(1300, max(2, int(round(H * rng.uniform(lo, hi)))))
            mode = LETTERBOX if k % 3 == 0 else STRETCH
            Z.append(_e(f"{cat} {sw}x{sh} -> {W}x{H}", [cat], (sw, sh), (W, H), mode, rot=bool(k % 2), swap=k % 5 == 0,
                        expect=MOD4 if res else FUSED))
    Z += [_e("down, width a multiple of 16", ["down"], (208, 150), 128), _e("down 7.5:1 x 1.5:1", ["down"], (480, 96), 64, rot=False)]
    # ---- Bayer: every pattern, W in {2, 4, 14, 16, 18, 30, 642}, H around the band, W * H % 16 in {0, 4, 8, 12}; 3 slots each
    B = [("RGGB", (2, 2), ID_GAINS), ("BGGR", (4, BAND + 2), SAT_GAINS), ("GRBG", (14, BAND - 2), ID_GAINS), ("GBRG", (16, BAND), ID_GAINS),
         ("RGGB", (18, 4), SAT_GAINS), ("BGGR", (30, 50), ID_GAINS), ("GBRG", (642, 482), ID_GAINS)]
    for i, (pat, (W, H), gains) in enumerate(B):
        hs = {2: "2", 4: "4", BAND - 2: "band-2", BAND: "band", BAND + 2: "band+2"}.get(H, "many")
        net = 128 if W > 100 else 64
        Z.append(_e(f"bayer {pat} {W}x{H}", ["bayer", f"bayer {pat}", f"bayer W={W}", f"bayer H={hs}", f"bayer WH%16={W * H % 16}",
                                              "bayer gains " + ("identity" if gains == ID_GAINS else "saturating")],
                    (W, H), net, rot=bool(i % 2), fmt=pat, gains=gains, expect=MOD4 if W % 4 else FUSED, slots=3))
    names = [z.name for z in Z]
    assert len(set(names)) == len(names), "entry names are the test ids: unique"
    return Z


# Minimum entries per category: at least 2 where the category is one condition, at least 1 per value of a listed set.
MINIMUM = {
    "identity": 2, "2:1": 2, "2:1 rot": 2, "3:1": 2, "4:1": 2, "down": 2, "stage limit": 2, "tap range": 2, "mild up": 2, "strong up": 2,
    "src 2": 1, "src 3": 1, "src 4": 1, "src 5": 1, "src 8": 1, "src 16": 1,
    "sw%4=0": 1, "sw%4=1": 1, "sw%4=2": 1, "sw%4=3": 1, "sw%16=0": 2, "sw%16!=0": 2, "sw=4096": 1, "sw=4095": 1,
    "pad x": 2, "pad y": 2, "pad odd": 2, "pad even": 2, "pad one column": 2, "pad one row": 2, "round .5": 2, "narrow box": 2,
    "slots=1": 2, "slots=3": 2, "tall source": 1,
    "bayer": 2, "bayer RGGB": 1, "bayer BGGR": 1, "bayer GRBG": 1, "bayer GBRG": 1,
    "bayer W=2": 1, "bayer W=4": 1, "bayer W=14": 1, "bayer W=16": 1, "bayer W=18": 1, "bayer W=30": 1, "bayer W=642": 1,
    "bayer H=2": 1, "bayer H=4": 1, "bayer H=band-2": 1, "bayer H=band": 1, "bayer H=band+2": 1, "bayer H=many": 1,
    "bayer WH%16=0": 1, "bayer WH%16=4": 1, "bayer WH%16=8": 1, "bayer WH%16=12": 1,
    "bayer gains identity": 1, "bayer gains saturating": 1,
}
REQUIRED_NAMES = ("up 2x2", "up 2x1200", "up 4096x2")

ZOO = build_zoo()

# The GPU test is parametrised by group, not by entry: a group is a few entries of related categories.
GROUPS = ("identity / integer ratios", "2:1 direct", "not fused", "strong up", "letterbox", "seeded", "bayer")


def group_of(e: Entry):
    c = e.cats
    if "bayer" in c:
        return "bayer"
    if "strong up" in c:
        return "strong up"
    if "2:1" in c:
        return "2:1 direct"
    if "down" in c or "mild up" in c:
        return "seeded"
    if e.expect != FUSED:
        return "not fused"
    if e.mode == LETTERBOX:
        return "letterbox"
    return "identity / integer ratios"
