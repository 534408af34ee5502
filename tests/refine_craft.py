"""Scenes and predictions for the refined point source (tests/test_refine.py, tests/test_gpu_refine.py).

Scenes: black frames with bright bars (3 - 5 px wide, 16 - 30 px tall, every one inside the light gates) and detections
whose boxes and keypoints are known exactly -- either a head written with write_head (keypoint columns per anchor), or a
whole step through a detect_craft blob whose stride-32 level lights all of its eight anchors with point-like boxes and one
armor-like quad each.  At 256 x 128 source pixels into a 128 x 64 net every coordinate is a small dyadic number: the
decode's fp32 arithmetic is exact and the closed forms below ARE what the engine reports (the GPU tests assert that).

Prediction: the guided extraction composed from the CPU oracle's own building blocks (orc_light_roi, orc_light_binary,
orc_find_external_contours, orc_contour_light) plus irmv_detection_amd.refine (guided_box, select, flag).

Test infrastructure only; never imported by the product package.
"""
from __future__ import annotations

import numpy as np

import detect_craft as dc
from irmv_detection_amd import refine
from oracle import oracle

SRC, NET = (256, 128), (128, 64)
FULL, WIN = (322, 201), (256, 128)          # tests/test_gpu_window.py's frame and window
QUAD = np.array([(-20, 12), (-20, -12), (20, -12), (20, 12)], np.float32)   # LB, LT, RT, RB around a plate's centre, source pixels
LIT_CLASS, LIT_LOGIT = 4, 2.0
MAX_CONTOURS, POINTS_CAP = 1024, 4096


# ---- the whole-step blob: eight plates -------------------------------------------------------------------------------
def plate_centres():
    """Centres of the eight stride-32 anchors of the 128 x 64 net, in pixels of a 256 x 128 source, in anchor order."""
    return [(32.0 + 64.0 * ix, 32.0 + 64.0 * iy) for iy in range(2) for ix in range(4)]


def step_blob(blob: bytes) -> bytes:
    """Level 2 lit on every anchor (one class, one logit), levels 0 and 1 dark; point-like boxes; the keypoints the quad
    QUAD around the anchor's centre: k_net = (2 v + i) 32 = (i + 0.5) 32 + d / 2  ->  v = (0.5 + d / 64) / 2."""
    from irmv_detection_amd import weights
    nc = weights.parse_blob(blob)[0]["nc"]
    lit = dc.dark_bias(nc, float(dc.DARK))
    lit[LIT_CLASS] = LIT_LOGIT
    dark = dc.dark_bias(nc, float(dc.DARK))
    kp = ((np.float32(0.5) + QUAD.reshape(8) / np.float32(64.0)) / np.float32(2.0)).astype(np.float32)
    return dc.craft(blob, cls={0: ("bias", dark), 1: ("bias", dark), 2: ("bias", lit)}, box=("bias", dc.POINT_BOXES), kpt=("bias", kp))


def step_detections(origin=(0.0, 0.0)):
    """(boxes float32 [8, 4], kpts float32 [8, 8]) the step_blob engine reports on a 256 x 128 source (or window at `origin`),
    in detection order (tied scores: anchor order)."""
    c = np.array(plate_centres(), np.float32) + np.array(origin, np.float32)
    boxes = np.concatenate([c, c], 1).astype(np.float32)
    kpts = (c[:, None, :] + QUAD[None]).reshape(8, 8).astype(np.float32)
    return boxes, kpts


# ---- frames ---------------------------------------------------------------------------------------------------------
def blank(size=SRC):
    return np.zeros((size[1], size[0], 3), np.uint8)


def bar(img, x0, y0, w, h, notch=True):
    """A filled bright rectangle: columns x0 .. x0 + w - 1, rows y0 .. y0 + h - 1, without its top-left pixel (notch): the
    simplified contour of a plain rectangle has four points, and a light needs five.  The minimum-area rectangle is the
    plain rectangle's all the same (the cut corner's edge spans a larger one) and runs through the outer pixels' centres:
    the light's ends are (x0 + (w - 1) / 2, y0) and (x0 + (w - 1) / 2, y0 + h - 1)."""
    assert 3 <= w <= 5 and 3 <= h <= 40 and x0 >= 0 and y0 >= 0 and x0 + w <= img.shape[1] and y0 + h <= img.shape[0], (x0, y0, w, h)
    img[y0:y0 + h, x0:x0 + w] = 255
    if notch:
        img[y0, x0] = 0


def bar_ends(x0, y0, w, h):
    """-> (bottom, top) of bar(x0, y0, w, h) as float32 pairs."""
    x = np.float32(x0) + np.float32(w - 1) / np.float32(2)
    return (x, np.float32(y0 + h - 1)), (x, np.float32(y0))


def plate_bars(img, centre, left=(0, 0), right=(0, 0), w=4, h=24, which="LR", origin=(0, 0)):
    """The two bars of a plate whose quad QUAD sits at `centre`: nominally the bars' ends lie half a pixel inside of the
    keypoints; left / right shift a bar by whole pixels.  -> [LB, LT, RT, RB] of the drawn bars (None where not drawn)."""
    cx, cy = int(centre[0]) + origin[0], int(centre[1]) + origin[1]
    out = [None] * 4
    if "L" in which:
        x0, y0 = cx - 22 + left[0], cy - 12 + left[1]
        bar(img, x0, y0, w, h)
        out[0], out[1] = bar_ends(x0, y0, w, h)
    if "R" in which:
        x0, y0 = cx + 19 + right[0], cy - 12 + right[1]
        bar(img, x0, y0, w, h)
        b, t = bar_ends(x0, y0, w, h)
        out[2], out[3] = t, b
    return out


def to_buffer(img, rotate180):
    """The frame as the producer writes it for an engine whose result coordinates are `img`'s."""
    return np.ascontiguousarray(img[::-1, ::-1]) if rotate180 else img


def step_scene(size=SRC, origin=(0, 0)):
    """The eight-plate frame of the whole-step cases, in result coordinates, and what each plate is:
       0, 1  both bars 1 - 3 px off the keypoints                         refined
       2     the left bar is missing                                      kept
       3     both bars 14 px down: beyond snap (and cut by the ROI)       kept
       4     both bars, and a third bright bar between them               refined (three lights)
       5     5 px wide bars, 22 tall                                      refined
       6     no bar at all                                                kept
       7     the right bar is a plain 3 x 3 blob (four contour points)    kept
    -> (img, expected flags)."""
    img = blank(size)
    c = plate_centres()
    plate_bars(img, c[0], left=(-1, 1), right=(1, -2), origin=origin)
    plate_bars(img, c[1], left=(1, -2), right=(-1, 1), h=26, origin=origin)
    plate_bars(img, c[2], which="R", origin=origin)
    plate_bars(img, c[3], left=(0, 14), right=(0, 14), origin=origin)
    plate_bars(img, c[4], left=(0, 1), right=(0, -1), origin=origin)
    bar(img, int(c[4][0]) + origin[0] - 2, int(c[4][1]) + origin[1] - 10, 4, 20)
    plate_bars(img, c[5], w=5, h=22, left=(0, 2), right=(-1, 1), origin=origin)
    plate_bars(img, c[7], which="L", origin=origin)
    bar(img, int(c[7][0]) + origin[0] + 19, int(c[7][1]) + origin[1], 3, 3, notch=False)
    return img, [1, 1, 0, 0, 1, 1, 0, 0]


# ---- prediction -----------------------------------------------------------------------------------------------------
def label_pool(cols, rows):
    """Bytes of an engine's label pool per slot for a cols x rows source frame."""
    return max(8 * cols * rows, (cols + 2) * (rows + 2) + 16)


def lights_of(img, gbox, params=None):
    """The guided ROI's lights from the oracle's blocks: -> (roi, no_answer, [(contour index, bottom, top)], contours)."""
    P = params or oracle.light_params()
    rows, cols = img.shape[:2]
    ok, roi, mn = oracle.light_roi(cols, rows, gbox)
    if not ok:
        return None, False, [], 0
    binary = oracle.light_binary(img, roi, P.binary_threshold)
    starts, pts = oracle.scan_external(binary)
    n = len(starts) - 1
    if n > MAX_CONTOURS or int(starts[-1]) > POINTS_CAP:
        return roi, True, [], n
    lights = []
    for c in range(n):
        p = pts[starts[c]:starts[c + 1]]
        if len(p) < 5:
            continue
        L = oracle.contour_light(p, P, (float(mn[0]), float(mn[1])))
        if L.ok:
            lights.append((c, (np.float32(L.bottom[0]), np.float32(L.bottom[1])), (np.float32(L.top[0]), np.float32(L.top[1]))))
    return roi, False, lights, n


def predict(img, boxes, kpts, snap=refine.DEFAULT_SNAP, margin=refine.DEFAULT_ROI_MARGIN, params=None, camera=None, plate=0):
    """What the guided extraction returns for detections (boxes, kpts) on the result-coordinate image `img`, one dict per
    detection: flag, n_lights, kpts (float32 [8]: the bars' ends where refined, else the inputs), roi, pool_offset.
    camera = (K, D): PnP's verdict on a chosen quad is the oracle's solver's (default: taken as solvable, which the GPU
    tests hold the engine to through pnp_ok == 1)."""
    rows, cols = img.shape[:2]
    pool, used, out = label_pool(cols, rows), 0, []
    for box, kp in zip(np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(kpts, np.float32).reshape(-1, 8)):
        rec = dict(flag=refine.KEPT, n_lights=0, kpts=kp.copy(), roi=None, pool_offset=used, lights=[])
        out.append(rec)
        g = refine.guided_box(box, kp, margin)
        if g is None:
            continue
        ok, roi, _ = oracle.light_roi(cols, rows, g)
        if not ok:
            continue
        rec["roi"] = roi
        need = refine.label_bytes(roi[2], roi[3])
        fits = used + need <= pool
        used += need
        if not fits:
            rec["flag"] = refine.flag(True, False)
            continue
        _, no_answer, lights, _ = lights_of(img, g, params)
        if no_answer:
            rec["flag"] = refine.flag(True, False)
            continue
        rec["n_lights"], rec["lights"] = len(lights), lights
        refined, iL, iR = refine.select(lights, kp, snap)
        if refined:
            by = {c: (b, t) for c, b, t in lights}
            (lb, lt), (rb, rt) = by[iL], by[iR]
            quad = np.array([lb[0], lb[1], lt[0], lt[1], rt[0], rt[1], rb[0], rb[1]], np.float32)
            pnp_ok = True if camera is None else oracle.solve_pnp_ippe(camera[0], camera[1], quad, plate)["ok"]
            rec["flag"] = refine.flag(False, True, pnp_ok)
            if pnp_ok:
                rec["kpts"] = quad
    return out
