"""Debug images on the host: irmv_detection_amd/render.py, the reference of irmv_engine_render (csrc/k_render.hip), against a
per-pixel scalar rendering written here from the rules of include/irmv_hip.h ("debug images") in Python integers, against
YoloEngine.visualize_bboxes, and the rasteriser's facts; plus what the C ABI answers without a GPU."""
import ctypes as C
import fractions
import itertools
import math
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from irmv_detection_amd import _build, capi, render
from irmv_detection_amd.engine import ArmorClass, YoloEngine, bbox
from render_zoo import INF, NAN, stacked, zoo

NAMES = [c.name for c in ArmorClass]     # B1 .. RS, UNKNOWN


# ---- the scalar reference -----------------------------------------------------------------------------------------------
def s_coord(v, org, s):
    v = float(np.float32(v))
    if math.isnan(v) or math.isinf(v) or abs(v) >= 16777216.0:
        return None
    return math.floor(fractions.Fraction(math.trunc(v) - org, s))


def s_box(px, py, x1, y1, x2, y2, w, h):
    cl = lambda v, hi: max(min(v, hi), 0)
    return ((py in (y1, y1 + 1, y2, y2 - 1) and cl(x1, w - 1) <= px <= cl(x2, w - 1)) or
            (px in (x1, x1 + 1, x2, x2 - 1) and cl(y1, h - 1) <= py <= cl(y2, h - 1)))


def s_label(px, py, text, x, y, cell):
    u, v = px - x, py - (y - 7 * cell)
    if u < 0 or v < 0 or v >= 7 * cell or u >= len(text) * 6 * cell:
        return False
    k, c, r = u // (6 * cell), (u % (6 * cell)) // cell, v // cell
    return c < 5 and bool((YoloEngine._GLYPHS[text[k]][r] >> (4 - c)) & 1)


def s_segment(px, py, a, b):
    dx, dy, qx, qy = b[0] - a[0], b[1] - a[1], px - a[0], py - a[1]
    L2, t = dx * dx + dy * dy, qx * dx + qy * dy
    if L2 == 0 or t < 0:
        return qx * qx + qy * qy <= 1
    if t > L2:
        return (px - b[0]) ** 2 + (py - b[1]) ** 2 <= 1
    return (qx * dy - qy * dx) ** 2 <= L2


def s_armor(px, py, pts, r):
    if any(abs((px - x) ** 2 + (py - y) ** 2 - r * r) <= 2 * r for x, y in pts):
        return True
    LB, LT, RT, RB = pts
    return any(s_segment(px, py, a, b) for a, b in ((LT, LB), (RT, RB), (LT, RT), (LB, RB)))


def scalar_render(img, kind, s, marks, dets, corner, T):
    H, W = img.shape[:2]
    ow, oh = W // s, H // s
    cell, r = {1: 3, 2: 2, 4: 1}[s], {1: 5, 2: 3, 4: 2}[s]
    recs = []
    for d in dets:
        xy = [s_coord(v, corner[i % 2], s) for i, v in enumerate(d["xyxy"])]
        kp = [s_coord(v, corner[i % 2], s) for i, v in enumerate(d["kpts"])]
        cls = d["class_id"]
        recs.append((None if None in xy else xy, None if (None in kp or d["armor_valid"] != 1) else list(zip(kp[0::2], kp[1::2])),
                     NAMES[cls] if 0 <= cls < 14 else "UNKNOWN", (0, 0, 255) if 0 <= cls <= 6 else (255, 0, 0)))
    out = np.zeros((oh, ow, 3), np.uint8)
    for y in range(oh):
        for x in range(ow):
            blk = [[int(c) for c in img[y * s + j, x * s + i]] for j in range(s) for i in range(s)]
            if kind == "color":
                px = [(sum(p[c] for p in blk) + s * s // 2) // (s * s) for c in range(3)]
            else:
                px = [255 * any(((p[0] * 3735 + p[1] * 19235 + p[2] * 9798 + (1 << 14)) >> 15) > T for p in blk)] * 3
            hit = None
            for xy, _, name, col in reversed(recs):
                if xy is not None and ((marks & 1 and s_box(x, y, *xy, ow, oh)) or (marks & 2 and s_label(x, y, name, xy[0], xy[1], cell))):
                    hit = col
                    break
            if hit is None and marks & 4 and any(pts is not None and s_armor(x, y, pts, r) for _, pts, _, _ in recs):
                hit = (0, 255, 0)
            out[y, x] = px if hit is None else hit
    return out


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(7).integers(0, 256, (16, 24, 3), dtype=np.uint8)


@pytest.mark.parametrize("kind,scale", list(itertools.product(("color", "binary"), (1, 2, 4))))
def test_render_equals_the_scalar_reference(image, kind, scale):
    dets = zoo(24, 16)
    for marks in range(8):
        got = render.render(image, kind, scale, marks, dets, binary_threshold=120)
        assert got.shape == (16 // scale, 24 // scale, 3) and got.dtype == np.uint8
        assert np.array_equal(got, scalar_render(image, kind, scale, marks, dets, (0, 0), 120)), (kind, scale, marks)


def test_many_stacked_records(image):
    dets = stacked(256)
    for scale in (1, 4):
        assert np.array_equal(render.render(image, "color", scale, 7, dets), scalar_render(image, "color", scale, 7, dets, (0, 0), 0))


@pytest.mark.parametrize("scale", (1, 2, 4))
def test_odd_sizes_drop_columns_and_rows_and_the_corner_is_subtracted(scale):
    img = np.random.default_rng(8).integers(0, 256, (15, 23, 3), dtype=np.uint8)
    dets = [dict(d, xyxy=tuple(v + (13 if i % 2 == 0 else 7) for i, v in enumerate(d["xyxy"])),
                 kpts=tuple(v + (13 if i % 2 == 0 else 7) for i, v in enumerate(d["kpts"]))) for d in zoo(23, 15)[:10]]
    for kind in ("color", "binary"):
        got = render.render(img, kind, scale, 7, dets, corner=(13, 7), binary_threshold=99)
        assert got.shape == (15 // scale, 23 // scale, 3)
        assert np.array_equal(got, scalar_render(img, kind, scale, 7, dets, (13, 7), 99))
    assert render.dims(23, 15, scale) == (23 // scale, 15 // scale)


def test_coordinates_truncate_then_floor():
    assert [render.coord(v, 0, 1) for v in (2.9, -2.9, -0.5, 0.0)] == [2, -2, 0, 0]
    assert [render.coord(v, 0, 2) for v in (3.9, -1.0, -3.9, -4.0)] == [1, -1, -2, -2]
    assert render.coord(5.9, 13, 4) == -2 and render.coord(20.0, 13, 4) == 1
    assert render.coord(16777215.0, 0, 1) == 16777215 and render.coord(16777216.0, 0, 1) is None and render.coord(-16777216.0, 0, 4) is None
    assert render.coord(NAN, 0, 1) is None and render.coord(INF, 0, 1) is None and render.coord(-INF, 0, 2) is None
    with pytest.raises(ValueError):
        render.dims(10, 10, 3)


def test_scale_one_boxes_and_labels_are_visualize_bboxes(image):
    dets = [d for d in zoo(24, 16) if render.coord(d["xyxy"][0], 0, 1) is not None and all(render.coord(v, 0, 1) is not None for v in d["xyxy"])]
    assert len(dets) >= 10
    exp = image.copy()
    fake = types.SimpleNamespace(src_image_size=(24, 16), _draw_label=YoloEngine._draw_label)
    YoloEngine.visualize_bboxes(fake, exp, [bbox(d["xyxy"], 0.5, ArmorClass(d["class_id"] if 0 <= d["class_id"] < 14 else 14)) for d in dets])
    assert np.array_equal(render.render(image, "color", 1, 3, dets), exp)
    assert not np.array_equal(exp, image)


def test_segment_is_symmetric_in_its_endpoints():
    rng = np.random.default_rng(9)
    for _ in range(200):
        a, b = (int(v) for v in rng.integers(-8, 40, 2)), (int(v) for v in rng.integers(-8, 40, 2))
        a, b = tuple(a), tuple(b)
        m = render.segment_mask((24, 32), a, b)
        assert np.array_equal(m, render.segment_mask((24, 32), b, a)), (a, b)
        ys, xs = np.nonzero(m)
        assert all(s_segment(int(x), int(y), a, b) for x, y in zip(xs, ys))
    far = render.segment_mask((24, 32), (-16777215, -16777215), (16777215, 16777215))   # the longest diagonal: products near 2^52
    assert np.array_equal(far, np.array([[abs(x - y) <= 1 for x in range(32)] for y in range(24)]))


def test_horizontal_segment_pixel_set():
    m = render.segment_mask((12, 20), (3, 5), (9, 5))
    exp = {(x, y) for x in range(3, 10) for y in (4, 5, 6)} | {(2, 5), (10, 5)}
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(m))} == exp
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(render.segment_mask((12, 20), (7, 7), (7, 7))))} == {(7, 7), (6, 7), (8, 7), (7, 6), (7, 8)}


def test_ring_of_radius_five():
    m = render.ring_mask((31, 31), 15, 15, 5)
    exp = np.array([[15 <= (x - 15) ** 2 + (y - 15) ** 2 <= 35 for x in range(31)] for y in range(31)])
    assert np.array_equal(m, exp) and m.sum() > 0
    for r in (3, 2):
        m = render.ring_mask((31, 31), 15, 15, r)
        assert np.array_equal(m, np.array([[abs((x - 15) ** 2 + (y - 15) ** 2 - r * r) <= 2 * r for x in range(31)] for y in range(31)]))
    assert render.RADIUS == {1: 5, 2: 3, 4: 2} and render.CELL == {1: 3, 2: 2, 4: 1}


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def test_glyphs_of_the_library_are_the_python_table(lib):
    for ch, rows in YoloEngine._GLYPHS.items():
        assert capi.render_glyph(ch) == tuple(rows), ch
    assert {ch for ch in map(chr, range(256)) if capi.render_glyph(ch) is not None} == set(YoloEngine._GLYPHS)
    assert set("".join(NAMES)) <= set(YoloEngine._GLYPHS)        # every name can be drawn


def test_host_only_argument_errors(lib):
    rows = (C.c_uint8 * 7)()
    assert lib.irmv_render_glyph(ord("A"), rows) == capi.ERR_ARG and lib.irmv_render_glyph(-1, rows) == capi.ERR_ARG
    assert lib.irmv_render_glyph(ord("B"), None) == capi.ERR_ARG
    assert lib.irmv_render_glyph(ord("B"), rows) == capi.OK
    w, h = C.c_int(0), C.c_int(0)
    assert lib.irmv_engine_render_dims(None, 0, 1, C.byref(w), C.byref(h)) == capi.ERR_ARG
    out = (C.c_uint8 * 16)()
    o = capi.render_opts()
    assert lib.irmv_engine_render(None, 0, C.byref(o), None, 0, out) == capi.ERR_ARG
    assert b"engine is null" in lib.irmv_last_error()


def test_render_opts_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in capi.RenderOpts._fields_]
    src = tmp_path / "ro.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu", sizeof(irmv_render_opts));' +
                   "".join(f'printf(" %zu", offsetof(irmv_render_opts, {f}));' for f in fields) +
                   'printf(" %d %d %u %u %u", IRMV_RENDER_COLOR, IRMV_RENDER_BINARY, IRMV_MARK_BOXES, IRMV_MARK_LABELS, IRMV_MARK_ARMORS);return 0;}\n')
    exe = tmp_path / "ro"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.RenderOpts)] + [getattr(capi.RenderOpts, f).offset for f in fields] + \
        [capi.RENDER_COLOR, capi.RENDER_BINARY, capi.MARK_BOXES, capi.MARK_LABELS, capi.MARK_ARMORS]
    assert (render.MARK_BOXES, render.MARK_LABELS, render.MARK_ARMORS) == (capi.MARK_BOXES, capi.MARK_LABELS, capi.MARK_ARMORS)
