"""The Bayer ISP on the host (no GPU): bayer.demosaic(algo="mhc") against a second reference written by the letter
(bayer_isp_ref.py), the folded gain / LUT table against the kernel's apply_gain, and the C ABI and facade surface of
irmv_engine_cfg.bayer_demosaic and irmv_engine_set_bayer_isp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bayer_isp_ref as ref
from conftest import ROOT
from irmv_detection_amd import _build, bayer, capi

PATTERNS = bayer.PATTERNS


# ---------------------------------------------------------------- MHC host reference
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", [(4, 4), (6, 4), (4, 10), (18, 10)])      # (W, H)
def test_mhc_matches_the_reference_by_the_letter(pattern, size):
    rng = np.random.default_rng(100 * size[0] + size[1])
    raw = rng.integers(0, 256, (size[1], size[0]), dtype=np.uint8)
    assert np.array_equal(bayer.demosaic(raw, pattern, algo="mhc"), ref.mhc_by_the_letter(raw, pattern))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_mhc_constant_colour_round_trips_exactly(pattern):
    rgb = np.empty((6, 8, 3), np.uint8)
    rgb[:] = (200, 17, 90)
    assert np.array_equal(bayer.demosaic(bayer.mosaic(rgb, pattern), pattern, algo="mhc"), rgb)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("axis", [0, 1])
def test_mhc_linear_ramp_is_exact_away_from_the_border(pattern, axis):
    # every mask sums to one and has no first moment: a linear ramp is reproduced where no tap is reflected
    n = 3 + 5 * np.arange(12)
    lin = np.broadcast_to(n[None, :] if axis == 1 else n[:10, None], (10, 12)).astype(np.uint8)
    got = bayer.demosaic(np.ascontiguousarray(lin), pattern, algo="mhc")
    assert np.array_equal(got[2:-2, 2:-2], np.repeat(lin[2:-2, 2:-2, None], 3, axis=2))
    assert np.array_equal(got, ref.mhc_by_the_letter(lin, pattern))


def _fin(s):
    return min(max((s + 8) >> 4, 0), 255)


def test_mhc_hand_computed_6x6_reflect101_at_every_edge():
    r = np.array([[10, 200, 30, 90, 50, 160],
                  [70, 20, 110, 40, 250, 60],
                  [130, 80, 150, 100, 170, 120],
                  [190, 140, 5, 220, 230, 180],
                  [15, 240, 35, 45, 55, 65],
                  [75, 85, 95, 105, 115, 125]], np.int64)
    d = bayer.demosaic(r.astype(np.uint8), "RGGB", algo="mhc")
    # (0,0), an R site.  Rows -1, -2 -> 1, 2; columns -1, -2 -> 1, 2.
    g = 8 * r[0, 0] + 4 * (r[1, 0] + r[1, 0] + r[0, 1] + r[0, 1]) - 2 * (r[2, 0] + r[2, 0] + r[0, 2] + r[0, 2])
    b = 12 * r[0, 0] + 4 * (r[1, 1] + r[1, 1] + r[1, 1] + r[1, 1]) - 3 * (r[2, 0] + r[2, 0] + r[0, 2] + r[0, 2])
    assert tuple(d[0, 0]) == (r[0, 0], _fin(g), _fin(b))
    # (0,5), G on the R row: R from W / E.  Columns 6, 7 -> 4, 3; rows -1, -2 -> 1, 2.
    red = (10 * r[0, 5] + 8 * (r[0, 4] + r[0, 4]) - 2 * (r[1, 4] + r[1, 4] + r[1, 4] + r[1, 4]) - 2 * (r[0, 3] + r[0, 3])
           + (r[2, 5] + r[2, 5]))
    blue = (10 * r[0, 5] + 8 * (r[1, 5] + r[1, 5]) - 2 * (r[1, 4] + r[1, 4] + r[1, 4] + r[1, 4]) - 2 * (r[2, 5] + r[2, 5])
            + (r[0, 3] + r[0, 3]))
    assert tuple(d[0, 5]) == (_fin(red), r[0, 5], _fin(blue))
    # (5,0), G on the B row: B from W / E.  Rows 6, 7 -> 4, 3; columns -1, -2 -> 1, 2.
    blue = (10 * r[5, 0] + 8 * (r[5, 1] + r[5, 1]) - 2 * (r[4, 1] + r[4, 1] + r[4, 1] + r[4, 1]) - 2 * (r[5, 2] + r[5, 2])
            + (r[3, 0] + r[3, 0]))
    red = (10 * r[5, 0] + 8 * (r[4, 0] + r[4, 0]) - 2 * (r[4, 1] + r[4, 1] + r[4, 1] + r[4, 1]) - 2 * (r[3, 0] + r[3, 0])
           + (r[5, 2] + r[5, 2]))
    assert tuple(d[5, 0]) == (_fin(red), r[5, 0], _fin(blue))
    # (5,5), a B site.  Rows 6, 7 -> 4, 3; columns 6, 7 -> 4, 3.
    g = 8 * r[5, 5] + 4 * (r[4, 5] + r[4, 5] + r[5, 4] + r[5, 4]) - 2 * (r[3, 5] + r[3, 5] + r[5, 3] + r[5, 3])
    red = 12 * r[5, 5] + 4 * (r[4, 4] + r[4, 4] + r[4, 4] + r[4, 4]) - 3 * (r[3, 5] + r[3, 5] + r[5, 3] + r[5, 3])
    assert tuple(d[5, 5]) == (_fin(red), _fin(g), r[5, 5])
    # (1,4), G on the B row, one pixel inside: only the distance-2 taps leave the frame.  Row -1 -> 1; column 6 -> 4.
    blue = (10 * r[1, 4] + 8 * (r[1, 3] + r[1, 5]) - 2 * (r[0, 3] + r[0, 5] + r[2, 3] + r[2, 5]) - 2 * (r[1, 2] + r[1, 4])
            + (r[1, 4] + r[3, 4]))
    red = (10 * r[1, 4] + 8 * (r[0, 4] + r[2, 4]) - 2 * (r[0, 3] + r[0, 5] + r[2, 3] + r[2, 5]) - 2 * (r[1, 4] + r[3, 4])
           + (r[1, 2] + r[1, 4]))
    assert tuple(d[1, 4]) == (_fin(red), r[1, 4], _fin(blue))
    # (4,1), G on the R row, one pixel inside.  Row 6 -> 4; column -1 -> 1.
    red = (10 * r[4, 1] + 8 * (r[4, 0] + r[4, 2]) - 2 * (r[3, 0] + r[3, 2] + r[5, 0] + r[5, 2]) - 2 * (r[4, 1] + r[4, 3])
           + (r[2, 1] + r[4, 1]))
    blue = (10 * r[4, 1] + 8 * (r[3, 1] + r[5, 1]) - 2 * (r[3, 0] + r[3, 2] + r[5, 0] + r[5, 2]) - 2 * (r[2, 1] + r[4, 1])
            + (r[4, 1] + r[4, 3]))
    assert tuple(d[4, 1]) == (_fin(red), r[4, 1], _fin(blue))
    # (2,2), an interior R site: no reflection at all
    g = 8 * r[2, 2] + 4 * (r[1, 2] + r[3, 2] + r[2, 1] + r[2, 3]) - 2 * (r[0, 2] + r[4, 2] + r[2, 0] + r[2, 4])
    b = 12 * r[2, 2] + 4 * (r[1, 1] + r[1, 3] + r[3, 1] + r[3, 3]) - 3 * (r[0, 2] + r[4, 2] + r[2, 0] + r[2, 4])
    assert tuple(d[2, 2]) == (r[2, 2], _fin(g), _fin(b))
    assert np.array_equal(d, ref.mhc_by_the_letter(r.astype(np.uint8), "RGGB"))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_mhc_clamps_at_both_ends(pattern):
    # one bright pixel on black: the negative lobes of the masks must come out as 0 ...
    raw = np.zeros((8, 8), np.uint8)
    raw[3, 4] = 255
    un = ref.mhc_unclamped(raw, pattern)
    got = bayer.demosaic(raw, pattern, algo="mhc")
    assert (un < 0).any()
    assert np.array_equal(got, np.clip(un, 0, 255))
    assert int((got == 0).sum()) == 181 and (got[un < 0] == 0).all()
    # ... and one black pixel on white: the same lobes overshoot 255 (the maximum of the clamped output says nothing here)
    raw = np.full((8, 8), 255, np.uint8)
    raw[3, 4] = 0
    un = ref.mhc_unclamped(raw, pattern)
    got = bayer.demosaic(raw, pattern, algo="mhc")
    assert (un > 255).any() and int(un.max()) > 255
    assert np.array_equal(got, np.clip(un, 0, 255)) and (got[un > 255] == 255).all()


def test_mhc_refuses_frames_below_4x4_and_unknown_algorithms():
    with pytest.raises(ValueError):
        bayer.demosaic(np.zeros((2, 8), np.uint8), "RGGB", algo="mhc")
    with pytest.raises(ValueError):
        bayer.demosaic(np.zeros((8, 2), np.uint8), "RGGB", algo="mhc")
    with pytest.raises(ValueError):
        bayer.demosaic(np.zeros((8, 8), np.uint8), "RGGB", algo="ahd")
    assert bayer.demosaic(np.zeros((2, 2), np.uint8), "RGGB").shape == (2, 2, 3)


# ---------------------------------------------------------------- the ISP table
def test_isp_table_with_identity_lut_is_apply_gain():
    for g in (0, 1, 255, 256, 300, 1023):
        t = bayer.isp_table((g, g, g))
        assert t.shape == (3, 256) and t.dtype == np.uint8
        for v in range(256):
            assert t[0, v] == t[1, v] == t[2, v] == ref.apply_gain(v, g), (g, v)
    assert np.array_equal(bayer.isp_table(), np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256)))
    assert np.array_equal(bayer.isp_table((256, 256, 256), np.arange(256, dtype=np.uint8)), bayer.isp_table())


def test_isp_table_folds_gains_and_lut():
    gam = ref.gamma_lut(0.5)
    assert gam[0] == 0 and gam[255] == 255 and gam[64] == 128
    t = bayer.isp_table(ref.GAINS, gam)
    per = np.stack([gam, 255 - gam, np.roll(gam, 7)])                    # a different curve per channel
    tp = bayer.isp_table(ref.GAINS, per)
    for c in range(3):
        for v in range(256):
            assert t[c, v] == gam[ref.apply_gain(v, ref.GAINS[c])]
            assert tp[c, v] == per[c][ref.apply_gain(v, ref.GAINS[c])]
    with pytest.raises(ValueError):
        bayer.isp_table((256, 256, 1024))
    with pytest.raises(ValueError):
        bayer.isp_table((256, 256, 256), np.zeros((2, 256), np.uint8))
    with pytest.raises(ValueError):
        bayer.isp_table((256, 256, 256), np.zeros(256, np.int32))


@pytest.mark.parametrize("algo", ["bilinear", "mhc"])
def test_table_after_either_algorithm_is_gains_then_lut(algo):
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, (12, 20), dtype=np.uint8)
    gam = ref.gamma_lut(0.5)
    per = np.stack([gam, 255 - gam, np.roll(gam, 7)])
    base = bayer.demosaic(raw, "GBRG", algo=algo)
    gained = bayer.demosaic(raw, "GBRG", ref.GAINS, algo)
    exp = np.minimum(255, (base.astype(np.int64) * np.array(ref.GAINS) + 128) >> 8)
    assert np.array_equal(gained, exp)
    assert np.array_equal(bayer.demosaic(raw, "GBRG", ref.GAINS, algo, gam), gam[exp])
    got = bayer.demosaic(raw, "GBRG", ref.GAINS, algo, per)
    assert all(np.array_equal(got[..., c], per[c][exp[..., c]]) for c in range(3))
    assert np.array_equal(got, bayer.isp_table(ref.GAINS, per)[np.arange(3), base])
    # the defaults are the arithmetic the existing callers get
    assert np.array_equal(bayer.demosaic(raw, "GBRG"), bayer.demosaic(raw, "GBRG", (256, 256, 256), "bilinear", None))


# ---------------------------------------------------------------- C ABI (no GPU needed)
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def _cfg(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    return cfg


def test_cfg_default_is_bilinear(lib):
    assert _cfg(lib).bayer_demosaic == capi.DEMOSAIC_BILINEAR == 0 and capi.DEMOSAIC_MHC == 1


@pytest.mark.parametrize("fmt,algo,size,needle", [
    (capi.SRC_BAYER_RGGB8, 2, (1280, 1024), b"bayer_demosaic"),
    (capi.SRC_HWC8, 2, (1280, 1024), b"bayer_demosaic"),
    (capi.SRC_BAYER_RGGB8, 65535, (1280, 1024), b"bayer_demosaic"),
    (capi.SRC_HWC8, capi.DEMOSAIC_MHC, (1280, 1024), b"needs a Bayer src_format"),
    (capi.SRC_BAYER_GRBG8, capi.DEMOSAIC_MHC, (2, 1024), b"src_width >= 4"),
    (capi.SRC_BAYER_GRBG8, capi.DEMOSAIC_MHC, (1280, 2), b"src_width >= 4"),
])
def test_bad_demosaic_configs_are_rejected_before_touching_the_gpu(lib, fmt, algo, size, needle):
    cfg = _cfg(lib)
    cfg.src_format, cfg.bayer_demosaic = fmt, algo
    cfg.src_width, cfg.src_height = size
    h = C.c_void_p()
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
    assert needle in lib.irmv_last_error(), lib.irmv_last_error()
    p = capi.FrontPlan()
    assert lib.irmv_front_plan(C.byref(cfg), C.byref(p)) == capi.ERR_ARG          # the same checks, in front of the plan
    # the same frame is no argument error for the bilinear kernel, nor a 4 x 4 one for MHC
    cfg.bayer_demosaic = capi.DEMOSAIC_BILINEAR
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) != capi.ERR_ARG
    cfg.src_format, cfg.bayer_demosaic, cfg.src_width, cfg.src_height = capi.SRC_BAYER_GRBG8, capi.DEMOSAIC_MHC, 4, 4
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) != capi.ERR_ARG, lib.irmv_last_error()


def test_callers_with_an_older_struct_size_get_bilinear(lib):
    """The field was reserved in the header of size offsetof(reserved2): whatever such a caller left there is not read."""
    old = capi.EngineCfg.reserved2.offset
    cfg = _cfg(lib)
    cfg.src_format, cfg.bayer_demosaic, cfg.struct_size = capi.SRC_BAYER_RGGB8, 7, old
    buf = C.create_string_buffer(bytes(C.string_at(C.addressof(cfg), old)), old)
    h = C.c_void_p()
    rc = lib.irmv_engine_create(C.cast(buf, C.POINTER(capi.EngineCfg)), C.byref(h))
    assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (rc, lib.irmv_last_error())
    cfg.struct_size = C.sizeof(capi.EngineCfg)
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG and b"bayer_demosaic" in lib.irmv_last_error()


def test_isp_entries_refuse_a_null_engine(lib):
    g = (C.c_uint16 * 3)(256, 256, 256)
    lut = (C.c_uint8 * 768)()
    assert lib.irmv_engine_set_bayer_isp(None, g, None) == capi.ERR_ARG
    assert b"null" in lib.irmv_last_error()
    assert lib.irmv_engine_set_bayer_isp(None, g, lut) == capi.ERR_ARG
    assert lib.irmv_engine_set_bayer_isp(None, None, None) == capi.ERR_ARG
    assert lib.irmv_engine_get_bayer_isp(None, g, lut) == capi.ERR_ARG
    assert list(g) == [256, 256, 256]


def test_bayer_demosaic_field_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n",'
                   'sizeof(irmv_engine_cfg), offsetof(irmv_engine_cfg, bayer_demosaic), sizeof(((irmv_engine_cfg *)0)->bayer_demosaic),'
                   'offsetof(irmv_engine_cfg, bayer_gain_q8), IRMV_DEMOSAIC_BILINEAR, IRMV_DEMOSAIC_MHC);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.EngineCfg), capi.EngineCfg.bayer_demosaic.offset, capi.EngineCfg.bayer_demosaic.size,
                   capi.EngineCfg.bayer_gain_q8.offset, capi.DEMOSAIC_BILINEAR, capi.DEMOSAIC_MHC]
    assert got[:3] == [280, 266, 2] and capi.EngineCfg.net_height.offset == 268


def test_reference_style_isp_code_compiles_against_the_facade():
    assert os.path.exists(ref.facade_exe())
