"""Frame metering on the host (include/irmv_hip.h, "frame metering"): the layouts against the header, the reference
irmv_detection_amd/metering.py against a brute-force double loop, irmv_meter_map against the reference, every refusal, the
four irmv_stats_* helpers against their Python twins, and the white-balance loop closed on the reference alone.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from irmv_detection_amd import _build, bayer, capi, metering, window

VIEW_SIZE = (12, 10)
# odd corners, partly outside on every side, wholly outside, one pixel, the whole view
RECTS = (None, (3, 1, 7, 6), (1, 3, 5, 5), (-3, -2, 8, 7), (7, 5, 20, 20), (5, 4, 1, 1), (0, 0, 12, 10), (12, 0, 3, 3), (-5, -5, 5, 5), (2, 11, 4, 2), (4, 3, 2, 1), (4, 3, 1, 2))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def test_layouts_match_the_header(tmp_path):
    structs = (("irmv_meter_opts", capi.MeterOpts), ("irmv_frame_stats", capi.FrameStats), ("irmv_meter_map_t", capi.MeterMap))
    parts = []
    for name, cls in structs:
        parts.append(f'printf(" %zu", sizeof({name}));')
        parts += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "mt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(parts) +
                   'printf(" %d %d", IRMV_METER_VIEW, IRMV_METER_RAW);return 0;}\n')
    exe = tmp_path / "mt"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    exp = []
    for _, cls in structs:
        exp += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == exp + [capi.METER_VIEW, capi.METER_RAW]
    assert C.sizeof(capi.FrameStats) % 16 == 0 and capi.FrameStats.n.offset == 4096


# ---- the reference against a double loop ---------------------------------------------------------------------------------
def brute(frame, rect, step, domain, rot, pattern=None, view_size=None, corner=(0, 0)):
    """The definition, pixel by pixel in RESULT coordinates (view) / site by site in buffer coordinates (raw)."""
    hist = np.zeros((4, 256), np.int64)
    vw, vh = (frame.shape[1], frame.shape[0]) if domain == "view" else view_size
    x0, y0, w, h = (0, 0, vw, vh) if rect is None else rect
    rx0, ry0, rx1, ry1 = max(x0, 0), max(y0, 0), min(x0 + w, vw), min(y0 + h, vh)
    if rx1 <= rx0 or ry1 <= ry0:
        return hist, (0, 0, 0, 0)
    if domain == "view":
        for y in range(ry0, ry1):
            for x in range(rx0, rx1):
                if (x - rx0) % step or (y - ry0) % step:
                    continue
                p = frame[vh - 1 - y, vw - 1 - x] if rot else frame[y, x]
                p0, p1, p2 = (int(v) for v in p)
                for r, v in enumerate((p0, p1, p2, (p0 * 3735 + p1 * 19235 + p2 * 9798 + (1 << 14)) >> 15)):
                    hist[r, v] += 1
        return hist, (rx0, ry0, rx1 - rx0, ry1 - ry0)
    # buffer coordinates of the clipped rectangle's pixels: flip inside the view, then the view's corner in the raw frame
    xs = sorted((vw - 1 - x if rot else x) + corner[0] for x in range(rx0, rx1))
    ys = sorted((vh - 1 - y if rot else y) + corner[1] for y in range(ry0, ry1))
    ex0, ex1 = xs[0] + (xs[0] & 1), (xs[-1] + 1) & ~1
    ey0, ey1 = ys[0] + (ys[0] & 1), (ys[-1] + 1) & ~1
    if ex1 <= ex0 or ey1 <= ey0:
        return hist, (0, 0, 0, 0)
    ry, rx = bayer._red_phase(pattern)
    for j in range((ey1 - ey0) // 2):
        for i in range((ex1 - ex0) // 2):
            if i % step or j % step:
                continue
            for dy in (0, 1):
                for dx in (0, 1):
                    y, x = ey0 + 2 * j + dy, ex0 + 2 * i + dx
                    v = int(frame[y, x])
                    colour = 0 if ((y & 1) == ry and (x & 1) == rx) else (2 if ((y & 1) != ry and (x & 1) != rx) else 1)
                    hist[colour, v] += 1
                    hist[3, v] += 1
    lx, ly = ex0 - corner[0], ey0 - corner[1]
    bw, bh = ex1 - ex0, ey1 - ey0
    return hist, ((vw - lx - bw, vh - ly - bh, bw, bh) if rot else (lx, ly, bw, bh))


def check_record(got, hist, rect, step, domain):
    assert np.array_equal(got["hist"], hist.astype(np.uint32))
    assert np.array_equal(got["n"], hist.sum(1)) and tuple(got["rect"]) == tuple(rect)
    assert (got["domain"], got["step"]) == (metering.DOMAINS[domain], step)


@pytest.mark.parametrize("rot", (True, False))
def test_view_reference_against_a_double_loop(rot):
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (VIEW_SIZE[1], VIEW_SIZE[0], 3), dtype=np.uint8)
    for rect, step in itertools.product(RECTS, (1, 2, 4)):
        hist, r = brute(f, rect, step, "view", rot)
        check_record(metering.meter(f, rect, step, "view", rot), hist, r, step, "view")
    assert metering.meter(f, (12, 0, 3, 3), 1, "view", rot)["hist"].sum() == 0


# a plain Bayer engine (the view is the frame), and 12 x 10 windows of a 16 x 14 frame at a corner of each parity
RAW_CASES = (((12, 10), (12, 10), None), ((16, 14), (12, 10), (0, 0)), ((16, 14), (12, 10), (1, 0)), ((16, 14), (12, 10), (2, 3)), ((16, 14), (12, 10), (3, 3)), ((16, 14), (12, 10), (4, 4)))


@pytest.mark.parametrize("rot", (True, False))
@pytest.mark.parametrize("pattern", bayer.PATTERNS)
def test_raw_reference_against_a_double_loop(pattern, rot):
    rng = np.random.default_rng(12)
    for full, view, win in RAW_CASES:
        raw = rng.integers(0, 256, (full[1], full[0]), dtype=np.uint8)
        corner = (0, 0) if win is None else window.buffer_origin(full, win[0], win[1], view[0], view[1], rot)
        for rect, step in itertools.product(RECTS, (1, 2, 4)):
            hist, r = brute(raw, rect, step, "raw", rot, pattern, view, corner)
            got = metering.meter(raw, rect, step, "raw", rot, pattern, view, corner)
            check_record(got, hist, r, step, "raw")
            n = got["n"]
            assert n[0] == n[2] and n[1] == 2 * n[0] and n[3] == 4 * n[0]


def test_meter_map_is_the_reference(lib):
    for rot, (rect, step) in itertools.product((True, False), itertools.product(RECTS, (1, 2, 4))):
        o = capi.meter_opts("view", rect, step)
        assert capi.meter_map(VIEW_SIZE, o, rotate180=rot) == metering.geometry(VIEW_SIZE, rect, step, "view", rot)
        for full, view, win in RAW_CASES:
            corner = (0, 0) if win is None else window.buffer_origin(full, win[0], win[1], view[0], view[1], rot)
            exp = metering.geometry(view, rect, step, "raw", rot, corner)
            o = capi.meter_opts("raw", rect, step)
            kw = dict(rotate180=rot, src_format="GRBG")
            got = capi.meter_map(full, o, capi.VIEW_WINDOW, None if win is None else view, win or (0, 0), **kw)
            assert got == exp, (rot, rect, step, full, win)
            if win is not None:   # the frame view of the same engine: the whole frame, no corner
                assert capi.meter_map(full, o, capi.VIEW_FRAME, view, win, **kw) == metering.geometry(full, rect, step, "raw", rot)
                ov = capi.meter_opts("view", rect, step)
                assert capi.meter_map(full, ov, capi.VIEW_WINDOW, view, win, **kw) == metering.geometry(view, rect, step, "view", rot)
    # a rectangle whose corner plus size passes 2^31
    o = capi.meter_opts("view", (5, 5, 2**31 - 1, 2**31 - 1), 1)
    assert capi.meter_map(VIEW_SIZE, o, rotate180=False)["rect"] == (5, 5, 7, 5)


def test_refusals_touch_no_gpu(lib):
    def call(o, src_format=capi.SRC_HWC8, view=0, window_=None, win_xy=(0, 0)):
        cfg = capi._geometry_cfg((16, 14), 64, None, capi.RESIZE_STRETCH, True, src_format, window_)
        m = capi.MeterMap()
        return lib.irmv_meter_map(C.byref(cfg), C.byref(o) if o is not None else None, view, win_xy[0], win_xy[1], C.byref(m))

    def opts(domain="view", rect=None, step=1, **kw):
        o = capi.meter_opts(domain, rect, step)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    assert call(opts()) == capi.OK and call(opts("raw"), "RGGB") == capi.OK
    bad = [opts(struct_size=0), opts(struct_size=C.sizeof(capi.MeterOpts) + 4), opts(domain=2), opts(domain=-1), opts(step=0), opts(step=3),
           opts(step=8), opts(step=-1), opts(rect=(0, 0, -1, 4)), opts(rect=(0, 0, 4, -1)), opts(rect=(0, 0, 0, 4)), opts(rect=(0, 0, 4, 0)),
           opts(reserved=0), opts(reserved=1)]
    for o in bad:
        assert call(o) == capi.ERR_ARG
        assert call(o, "RGGB") == capi.ERR_ARG
    assert call(opts("raw")) == capi.ERR_ARG and b"IRMV_METER_RAW" in lib.irmv_last_error()      # RAW on IRMV_SRC_HWC8
    assert call(None) == capi.ERR_ARG
    assert call(opts(), view=2) == capi.ERR_ARG and call(opts(), view=capi.VIEW_FRAME) == capi.ERR_ARG   # no window: no frame view
    assert call(opts(), window_=(12, 10), win_xy=(5, 0)) == capi.ERR_ARG                                # the window leaves the frame
    assert call(opts(), window_=(12, 10), win_xy=(4, 4), view=capi.VIEW_FRAME) == capi.OK
    cfg = capi._geometry_cfg((16, 14), 64, None, capi.RESIZE_STRETCH, True, capi.SRC_HWC8, None)
    assert lib.irmv_meter_map(C.byref(cfg), C.byref(opts()), 0, 0, 0, None) == capi.ERR_ARG
    assert lib.irmv_meter_map(None, C.byref(opts()), 0, 0, 0, C.byref(capi.MeterMap())) == capi.ERR_ARG
    # the engine entries check their engine before anything else
    s = capi.FrameStats()
    assert lib.irmv_engine_meter(None, 0, C.byref(opts()), C.byref(s)) == capi.ERR_ARG
    assert lib.irmv_engine_set_metering(None, C.byref(opts())) == capi.ERR_ARG
    assert lib.irmv_engine_frame_stats(None, 0, C.byref(s)) == capi.ERR_ARG
    assert lib.irmv_meter_limits(None) == capi.ERR_ARG
    L = capi.meter_limits()
    assert L["rows_per_block"] >= 1 and L["blocks_max"] >= 3 and L["threads"] % 64 == 0 and L["lds_bytes"] == L["threads"] // 64 * 4 * 256 * 4


# ---- the helpers ---------------------------------------------------------------------------------------------------------
def seeded_stats(seed, scale=1 << 20, domain=1):
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, scale, (4, 256), dtype=np.int64)
    hist[:, rng.integers(0, 256, 40)] = 0
    return dict(hist=hist.astype(np.uint32), n=hist.sum(1).astype(np.uint64), rect=(0, 0, 0, 0), domain=domain, step=1)


def near_2_32():
    """Counts near 2^32 in every bin: S N products pass 2^64 (n itself does not fit the record's uint32 and is unused here)."""
    hist = np.full((4, 256), 2**32 - 1, np.int64)
    hist[0] -= np.arange(256)
    hist[2, :128] = 2**31
    return dict(hist=hist.astype(np.uint32), n=np.array([2**32 - 1] * 4, np.uint64), rect=(0, 0, 0, 0), domain=1, step=1)


def either(fn_c, fn_py, *a):
    """Both answers, a refusal as None: the C helper and its Python twin must agree on which it is."""
    try:
        py = fn_py(*a)
    except ValueError:
        py = None
    try:
        c = fn_c(*a)
    except capi.IrmvError as e:
        assert e.code == capi.ERR_ARG
        c = None
    return c, py


def test_helpers_equal_their_python_twins(lib):
    ranges = ((0, 255), (8, 247), (100, 100), (200, 100), (255, 255), (0, 0))
    fractions = ((0, 1), (1, 1), (1, 2), (1, 100), (99, 100), (999, 1000), (1, 3))
    for st in [seeded_stats(s) for s in range(4)] + [seeded_stats(9, 3), near_2_32()]:
        for row, (lo, hi) in itertools.product(range(4), ranges):
            c, py = either(capi.stats_mean_q8, metering.mean_q8, st, row, lo, hi)
            assert c == py and c is not None
        for row, (num, den) in itertools.product(range(4), fractions):
            c, py = either(capi.stats_percentile, metering.percentile, st, row, num, den)
            assert c == py and c is not None
            for target in (0, 1, 120, 255):
                c, py = either(capi.stats_exposure_q8, metering.exposure_q8, st, row, num, den, target)
                assert c == py and c is not None
        for lo, hi in ranges:
            c, py = either(capi.stats_gray_world, metering.gray_world, st, lo, hi)
            assert c == py
    big = near_2_32()
    assert metering.mean_q8(big, 0, 0, 255)[1] > 2**39 and capi.stats_gray_world(big, 0, 255) == metering.gray_world(big, 0, 255)


def test_helper_edges(lib):
    st = seeded_stats(5)
    assert capi.stats_mean_q8(st, 1, 200, 100) == (0, 0) == metering.mean_q8(st, 1, 200, 100)       # an empty range
    empty = dict(hist=np.zeros((4, 256), np.uint32), n=np.zeros(4, np.uint32), rect=(0, 0, 0, 0), domain=1, step=1)
    assert capi.stats_mean_q8(empty, 0) == (0, 0)
    for fn_c, fn_py, a in ((capi.stats_percentile, metering.percentile, (empty, 0, 1, 2)), (capi.stats_exposure_q8, metering.exposure_q8, (empty, 3, 1, 2, 100)),
                           (capi.stats_gray_world, metering.gray_world, (empty, 8, 247))):
        assert either(fn_c, fn_py, *a) == (None, None)                                              # n == 0
    zero = dict(empty, hist=np.zeros((4, 256), np.uint32))
    zero["hist"][:, 0] = 1000                                                                       # all mass in bin 0
    zero["n"] = np.full(4, 1000, np.uint32)
    g = (C.c_uint16 * 3)(7, 8, 9)
    assert lib.irmv_stats_gray_world(C.byref(capi.stats_struct(zero)), 0, 255, g) == capi.ERR_ARG and tuple(g) == (7, 8, 9)
    assert either(capi.stats_gray_world, metering.gray_world, zero, 0, 255) == (None, None)
    assert capi.stats_percentile(zero, 0, 1, 1) == 0 and capi.stats_exposure_q8(zero, 0, 1, 1, 255) == 4096 == metering.exposure_q8(zero, 0, 1, 1, 255)
    assert capi.stats_exposure_q8(zero, 0, 1, 1, 0) == 16
    dark = dict(empty, hist=np.zeros((4, 256), np.uint32))                                          # R and B a tenth of G: the 1023 clamp
    dark["hist"][0, 20] = dark["hist"][2, 20] = 100
    dark["hist"][1, 200] = 200
    dark["n"] = np.array([100, 200, 100, 400], np.uint32)
    assert capi.stats_gray_world(dark, 8, 247) == (1023, 256, 1023) == metering.gray_world(dark, 8, 247)
    one = dict(empty, hist=np.zeros((4, 256), np.uint32), n=np.array([10, 0, 0, 0], np.uint32))
    one["hist"][0, 37] = 4
    one["hist"][0, 90] = 6
    assert [capi.stats_percentile(one, 0, n, 10) for n in (0, 1, 4, 5, 10)] == [0, 37, 37, 90, 90]   # num = 0: the smallest v at all
    assert [metering.percentile(one, 0, n, 10) for n in (0, 1, 4, 5, 10)] == [0, 37, 37, 90, 90]
    view_rec = dict(st, domain=0)
    assert either(capi.stats_gray_world, metering.gray_world, view_rec, 8, 247) == (None, None)     # RAW records only
    s = capi.stats_struct(st)
    m, n, v = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    for row, lo, hi in ((-1, 0, 255), (4, 0, 255), (0, -1, 255), (0, 0, 256)):
        assert lib.irmv_stats_mean_q8(C.byref(s), row, lo, hi, C.byref(m), C.byref(n)) == capi.ERR_ARG
    assert lib.irmv_stats_percentile(C.byref(s), 0, 2, 1, C.byref(v)) == capi.ERR_ARG and lib.irmv_stats_percentile(C.byref(s), 0, 0, 0, C.byref(v)) == capi.ERR_ARG
    assert lib.irmv_stats_exposure_q8(C.byref(s), 0, 1, 2, 256, C.byref(v)) == capi.ERR_ARG
    assert lib.irmv_stats_mean_q8(None, 0, 0, 255, C.byref(m), C.byref(n)) == capi.ERR_ARG


# ---- white balance closes on the reference alone -------------------------------------------------------------------------
def tinted_scene(pattern, seed=21, size=(100, 68)):
    """A seeded gray image in [40, 200), tinted to (0.6, 1, 0.8) and mosaiced: what a sensor under a warm light hands over."""
    rng = np.random.default_rng(seed)
    gray = rng.integers(40, 200, (size[1], size[0])).astype(np.float64)
    rgb = np.stack([np.floor(gray * 0.6 + 0.5), gray, np.floor(gray * 0.8 + 0.5)], axis=2).astype(np.uint8)
    return bayer.mosaic(rgb, pattern)


@pytest.mark.parametrize("pattern", bayer.PATTERNS)
def test_white_balance_closes_on_the_reference(pattern):
    raw = tinted_scene(pattern)
    st = metering.meter(raw, None, 1, "raw", True, pattern)
    gains = metering.gray_world(st, 8, 247)
    assert gains[1] == 256 and gains[0] > 256 and gains[2] > 256
    out = bayer.demosaic(raw, pattern, gains)
    means = out.reshape(-1, 3).mean(0)
    print(pattern, "gains", gains, "means", means, "spread", means.max() - means.min())
    assert means.max() - means.min() < 1.0
    plain = bayer.demosaic(raw, pattern).reshape(-1, 3).mean(0)
    assert plain.max() - plain.min() > 20.0                  # the tint was there
