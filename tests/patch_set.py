"""The seeded inputs of the plate-patch tests (tests/test_patches.py, tests/test_gpu_patches.py): the 128 x 96 frames, the
quad set whose every quantisation stands at least 1e-9 of a step away from flipping (asserted on the CPU, so that the GPU test
can demand bytes of all of them), the hard quads, and the step fixture.

Test infrastructure only; never imported by the product package.
"""
from __future__ import annotations

import functools

import numpy as np

from irmv_detection_amd import patches as PT

SRC, NET = (128, 96), (64, 64)          # source (W, H), net (W, H)
SEED, N_QUADS = 23, 400
MARGIN = 1e-9                            # of a quantisation step (1 / 32 px); the host / device discrepancy is of order 1e-13
STEP_THR, STEP_MAX_DET = 0.25, 100       # the step tests' score threshold and the engine's default max_det
STEP_MIN = 8


@functools.lru_cache(maxsize=None)
def frame(seed: int = 0, size=SRC) -> np.ndarray:
    """A seeded frame in result coordinates: smooth structure (so that neighbouring texels differ and bilinear weights
    matter) plus noise, every channel its own.  Read-only."""
    r = np.random.RandomState(1000 + seed)
    W, H = size
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3), np.float64)
    for c in range(3):
        fx, fy, ph = r.uniform(0.05, 0.4), r.uniform(0.05, 0.4), r.uniform(0, 6.28)
        img[..., c] = 127.5 + 90.0 * np.sin(fx * x + fy * y + ph) + r.uniform(-37, 37, (H, W))
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def rect_quad(lt, w, h) -> np.ndarray:
    """LB, LT, RT, RB of the axis-parallel rectangle with left-top corner lt."""
    x, y = lt
    return np.array([x, y + h, x, y, x + w, y, x + w, y + h], np.float32)


@functools.lru_cache(maxsize=None)
def quad_set():
    """(kpts float32 [N, 8], sizes int32 [N]): centre within 20 px of the frame's, width 8 .. 50, height 4 .. 24, 1 px of
    noise on every corner, both plate sizes alternating."""
    r = np.random.RandomState(SEED)
    k = np.empty((N_QUADS, 8), np.float32)
    for i in range(N_QUADS):
        cx, cy = SRC[0] / 2 + r.uniform(-20, 20), SRC[1] / 2 + r.uniform(-20, 20)
        w, h = r.uniform(8, 50), r.uniform(4, 24)
        q = np.array([cx - w / 2, cy + h / 2, cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
        k[i] = (q + r.uniform(-1, 1, 8)).astype(np.float32)
    sizes = (np.arange(N_QUADS) & 1).astype(np.int32)
    k.setflags(write=False); sizes.setflags(write=False)
    return k, sizes


@functools.lru_cache(maxsize=None)
def quad_set_reference():
    """patches.patch of every quad of the set on frame(0), computed once."""
    k, s = quad_set()
    return tuple(PT.patch(frame(0), k[i], int(s[i])) for i in range(len(k)))


def hard_quads():
    """[(name, kpts float32 [8], size, opts or None, frame seed or ("level", v), state the case is built for or None)] --
    every one against the reference."""
    W, H = SRC
    inf, nan = np.inf, np.nan
    base = rect_quad((40, 30), 31, 12)
    out = []

    def add(name, k, size=0, opts=None, fr=0, state=None):
        out.append((name, np.asarray(k, np.float32).reshape(8), size, opts, fr, state))

    add("repeated point (RT == RB)", [40, 42, 40, 30, 71, 30, 71, 30], state=0)      # den == 0
    add("all one point", [50, 50] * 4, state=0)
    add("collinear", [10, 10, 20, 20, 30, 30, 40, 40], state=0)
    add("RT, RB, LB collinear", [40, 60, 40, 30, 60, 60, 50, 60], state=0)
    for name, v in (("nan", nan), ("+inf", inf), ("-inf", -inf)):
        for pos in (0, 5):
            k = base.copy(); k[pos] = v
            add(f"{name} at {pos}", k, state=0)
    for pos in (0, 5):
        k = base.copy(); k[pos] = 1e30
        add(f"1e30 at {pos}", k)
    add("all 1e30", [1e30, 1e30, 1e30, -1e30, -1e30, -1e30, -1e30, 1e30])
    # w = (g s + h t) + 1 with t in [-7/12, 20/12]: a bottom edge four times the top one has h = -3/4, w < 0 in the last rows;
    # a top edge 3.75 times the bottom one has h = 2.75, w < 0 in the first rows
    add("horizon inside the patch, below", [40, 50, 55, 30, 65, 30, 80, 50], state=0)
    add("horizon inside the patch, above", [52, 45, 30, 30, 90, 30, 68, 45], size=1, state=0)
    add("wholly outside, left", rect_quad((-400, 30), 31, 12), state=1)
    add("wholly outside, below", rect_quad((40, 500), 31, 12), size=1, state=1)
    for name, lt in (("left edge", (-12, 40)), ("right edge", (W - 16, 40)), ("top edge", (50, -7)), ("bottom edge", (50, H - 9)),
                     ("corner LT", (-15, -6)), ("corner RT", (W - 14, -5)), ("corner LB", (-13, H - 8)), ("corner RB", (W - 17, H - 7))):
        k = rect_quad(lt, 31.3, 12.6)
        k[[2, 4]] += 0.37; k[[1, 7]] -= 0.21
        add(f"crossing the {name}", k, size=len(name) & 1, state=1)
    add("1-pixel quad", rect_quad((60.3, 40.6), 1, 1), state=1)
    add("1e6-pixel quad", rect_quad((-5e5 + 0.4, -5e5 + 0.7), 1e6, 1e6), size=1, state=1)
    add("one-level frame", base, fr=("level", 93), state=1)
    add("one-level frame, black", base, size=1, fr=("level", 0), state=1)
    add("one-level frame, white", base, fr=("level", 255), state=1)
    tilt = np.array([38.2, 47.9, 41.1, 29.6, 83.4, 33.3, 80.7, 52.2], np.float32)
    for opts in (dict(span=(20, 128)), dict(span=(128, 20)), dict(light_rows=1), dict(light_rows=28), dict(top=0), dict(top=27),
                 dict(span=(22, 126), light_rows=28, top=27), dict(span=(126, 22), light_rows=1, top=0)):
        for size in (0, 1):
            add(f"options {opts}", tilt, size=size, opts=opts, state=1)
    return out


def hard_frame(fr) -> np.ndarray:
    if isinstance(fr, tuple):
        return np.full((SRC[1], SRC[0], 3), fr[1], np.uint8)
    return frame(fr)


# ---- the step fixture ---------------------------------------------------------------------------------------------------
def step_frame(seed: int = 0) -> np.ndarray:
    """The step tests' frames in result coordinates (three different ones: seeds 0, 1, 2)."""
    return frame(10 + seed)


def to_buffer(img, rotate180):
    """The frame as the producer writes it for an engine whose result coordinates are `img`'s."""
    return np.ascontiguousarray(img[::-1, ::-1]) if rotate180 else np.ascontiguousarray(img)


def fields(p) -> dict:
    """A capi.PlatePatch as the reference's dict."""
    return dict(gray=np.frombuffer(bytes(p), np.uint8, PT.PATCH_N).reshape(PT.PATCH_H, PT.PATCH_W), state=p.state, otsu=p.otsu,
                n_outside=p.n_outside, armor_size=p.armor_size, bar_sum=(p.bar_sum[0], p.bar_sum[1]), sum=p.sum)


def same(got: dict, want: dict) -> bool:
    return (np.array_equal(got["gray"], want["gray"]) and
            all(got[k] == want[k] for k in ("state", "otsu", "n_outside", "armor_size", "sum")) and tuple(got["bar_sum"]) == tuple(want["bar_sum"]))
