"""Tracking window, host side: the appended configuration fields and their validation, irmv_window_map against its numpy
statement (irmv_detection_amd/window.py), the front's plan of a window engine, and the C++ facade.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, K_REF
from irmv_detection_amd import _build, capi, window

FULL, WIN = (322, 201), (256, 128)
ORIGINS = [(0, 0), (66, 0), (0, 73), (66, 73), (31, 40)]   # the four corners and an interior corner


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def _cfg(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    return cfg


def test_cfg_default_has_no_window(lib):
    cfg = _cfg(lib)
    assert cfg.struct_size == C.sizeof(capi.EngineCfg)
    assert cfg.win_width == 0 and cfg.win_height == 0
    # the two fields follow reserved2 and fill the struct's former tail padding: its size is what it was before them
    assert capi.EngineCfg.win_width.offset == capi.EngineCfg.reserved2.offset + 4
    assert capi.EngineCfg.win_height.offset + 2 == C.sizeof(capi.EngineCfg)


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(irmv_engine_cfg), offsetof(irmv_engine_cfg, win_width), offsetof(irmv_engine_cfg, win_height),'
                   'sizeof(irmv_window_map_t), offsetof(irmv_window_map_t, band_offset), offsetof(irmv_window_map_t, cx));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.EngineCfg), capi.EngineCfg.win_width.offset, capi.EngineCfg.win_height.offset,
                   C.sizeof(capi.WindowMap), capi.WindowMap.band_offset.offset, capi.WindowMap.cx.offset]


def test_previous_struct_sizes_are_accepted_until_the_gpu_is_needed(lib):
    """The header before the window fields had this struct's size; the two older ones are shorter.  All three reach the
    point where the GPU is needed, and the older two never have a window whatever lies behind their end."""
    h = C.c_void_p()
    sizes = [capi.EngineCfg.src_format.offset, capi.EngineCfg.reserved2.offset, C.sizeof(capi.EngineCfg)]
    for old in sizes:
        cfg = _cfg(lib)
        cfg.weights_path = b"/nonexistent/model.irmw"
        cfg.struct_size = old
        if old != C.sizeof(capi.EngineCfg):
            cfg.win_width, cfg.win_height = -7, 30000        # not read: such a caller's struct ends before them
        rc = lib.irmv_engine_create(C.byref(cfg), C.byref(h))
        assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (old, rc, lib.irmv_last_error())
        assert b"size" not in lib.irmv_last_error() and b"win_" not in lib.irmv_last_error()
    cfg.struct_size = capi.EngineCfg.win_width.offset         # the end of reserved2 is no struct size of any header
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
    assert b"size mismatch" in lib.irmv_last_error()


@pytest.mark.parametrize("w,h,needle", [
    (640, 0, b"win_height"),          # exactly one of them zero
    (0, 512, b"win_width"),
    (1281, 512, b"win_width"),        # wider than the frame
    (640, 1025, b"win_height"),       # taller than the frame
    (-1, 512, b"win_width"),          # negative
    (640, -1, b"win_height"),
])
def test_bad_window_configs_are_rejected_before_touching_the_gpu(lib, w, h, needle):
    cfg = _cfg(lib)
    cfg.weights_path = b"/nonexistent/model.irmw"
    cfg.win_width, cfg.win_height = w, h
    hd = C.c_void_p()
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(hd)) == capi.ERR_ARG
    assert needle in lib.irmv_last_error(), lib.irmv_last_error()
    p = capi.FrontPlan()
    assert lib.irmv_front_plan(C.byref(cfg), C.byref(p)) == capi.ERR_ARG
    # the largest and the smallest window pass the configuration checks
    for ok in ((1280, 1024), (1, 1)):
        cfg.win_width, cfg.win_height = ok
        rc = lib.irmv_engine_create(C.byref(cfg), C.byref(hd))
        assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (ok, rc, lib.irmv_last_error())


def test_a_bayer_window_engine_needs_an_even_full_frame_only(lib):
    cfg = _cfg(lib)
    cfg.src_format = capi.SRC_BAYER_GRBG8
    cfg.src_width, cfg.src_height = 322, 202
    cfg.win_width, cfg.win_height = 255, 127          # any size: the crop comes after the demosaic
    p = capi.FrontPlan()
    assert lib.irmv_front_plan(C.byref(cfg), C.byref(p)) == capi.OK
    cfg.src_height = 201
    assert lib.irmv_front_plan(C.byref(cfg), C.byref(p)) == capi.ERR_ARG and b"even" in lib.irmv_last_error()


@pytest.mark.parametrize("rot", [True, False])
def test_window_map_matches_the_numpy_statement(lib, rot):
    K = list(K_REF)
    for x0, y0 in ORIGINS:
        got = capi.window_map(FULL, WIN, x0, y0, rot, K, net_size=128, net_height=64)
        exp = window.window_map(FULL, WIN, x0, y0, rot, K)
        assert got == exp, ((x0, y0), got, exp)
        # stated once more, by hand
        bx0, by0 = (FULL[0] - x0 - WIN[0], FULL[1] - y0 - WIN[1]) if rot else (x0, y0)
        assert (got["bx0"], got["by0"]) == (bx0, by0)
        assert got["band_offset"] == by0 * FULL[0] * 3 and got["band_bytes"] == WIN[1] * FULL[0] * 3
        assert got["band_offset"] + got["band_bytes"] <= FULL[0] * FULL[1] * 3
        # the principal point, bit for bit
        assert np.float64(got["cx"]).tobytes() == (np.float64(K[2]) - np.float64(x0)).tobytes()
        assert np.float64(got["cy"]).tobytes() == (np.float64(K[5]) - np.float64(y0)).tobytes()
    for x0, y0 in [(-1, 0), (0, -1), (67, 0), (0, 74), (67, 74)]:   # one pixel outside on each side
        with pytest.raises(capi.IrmvError) as ei:
            capi.window_map(FULL, WIN, x0, y0, rot, K, net_size=128, net_height=64)
        assert ei.value.code == capi.ERR_ARG
        with pytest.raises(ValueError):
            window.window_map(FULL, WIN, x0, y0, rot, K)


def test_window_map_needs_a_window(lib):
    cfg = _cfg(lib)
    m = capi.WindowMap()
    assert lib.irmv_window_map(C.byref(cfg), 0, 0, C.byref(m)) == capi.ERR_ARG
    assert b"window" in lib.irmv_last_error()
    assert lib.irmv_window_map(None, 0, 0, C.byref(m)) == capi.ERR_ARG
    assert lib.irmv_engine_set_window(None, 0, 0, 0) == capi.ERR_ARG
    assert lib.irmv_engine_get_window(None, 0, None, None, None, None) == capi.ERR_ARG


@pytest.mark.parametrize("full,win,net,mode,rot", [
    ((1280, 1024), (640, 512), (640, 512), capi.RESIZE_STRETCH, True),       # 1 : 1
    ((322, 201), (256, 128), (128, 64), capi.RESIZE_STRETCH, True),          # exactly 2 : 1, direct tiles
    ((322, 201), (256, 128), (128, 64), capi.RESIZE_STRETCH, False),
    ((1280, 1024), (642, 480), (640, 640), capi.RESIZE_LETTERBOX, True),     # win_width % 4 != 0: the front's fallback
    ((1281, 1023), (640, 480), (640, 640), capi.RESIZE_LETTERBOX, False),    # an odd full frame does not reach the front
])
def test_front_plan_of_a_window_config_is_the_plan_of_the_window_sized_source(lib, full, win, net, mode, rot):
    a = capi.front_plan(full, net[0], net[1], mode, rot, window=win)
    b = capi.front_plan(win, net[0], net[1], mode, rot)
    assert a == b
    if win[0] % 4:
        assert not a["fused"] and a["reason"] == capi.FRONT_WIDTH_MOD4


@pytest.mark.parametrize("rot", [True, False])
def test_crop_of_a_rotated_frame_is_the_rotated_crop(rot):
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (FULL[1], FULL[0], 3), dtype=np.uint8)
    for x0, y0 in ORIGINS:
        c = window.crop(f, x0, y0, WIN[0], WIN[1], rot)
        assert c.shape == (WIN[1], WIN[0], 3) and c.flags["C_CONTIGUOUS"]
        if rot:
            assert np.array_equal(c[::-1, ::-1], f[::-1, ::-1][y0:y0 + WIN[1], x0:x0 + WIN[0]])
        else:
            assert np.array_equal(c, f[y0:y0 + WIN[1], x0:x0 + WIN[0]])
        # the bytes irmv_window_map's band holds are the rows the crop reads
        m = window.window_map(FULL, WIN, x0, y0, rot)
        band = f.reshape(-1)[m["band_offset"]:m["band_offset"] + m["band_bytes"]].reshape(WIN[1], FULL[0], 3)
        assert np.array_equal(band[:, m["bx0"]:m["bx0"] + WIN[0]], c)
    assert window.shifted_camera(K_REF, 31, 40)[2] == K_REF[2] - 31.0 and window.shifted_camera(K_REF, 31, 40)[5] == K_REF[5] - 40.0


FACADE_SRC = r"""
#include <cstdio>
#include <cstring>
#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/yolo_engine.hpp"

int main(int argc, char ** argv)
{
  if (argc < 3) return 2;
  // the full 1280 x 1024 frame goes in, the network runs on a 640 x 512 window of it at the sensor's resolution
  irmv_detection::YoloEngine engine(argv[1], cv::Size(1280, 1024), true, -1, false, 640, IRMV_SRC_HWC8, {256, 256, 256}, 512,
                                    IRMV_DEMOSAIC_BILINEAR, cv::Size(640, 512));
  FILE * f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  const size_t n = std::fread(engine.get_src_image_buffer(), 1, engine.src_image_bytes(), f);
  std::fclose(f);
  if (n != engine.src_image_bytes()) return 4;
  const auto w0 = engine.window();
  auto bboxes = engine.detect();
  // follow the last detection: the window around its box centre, clamped into the frame
  cv::Point2f c(1270.f, 5.f);
  if (!bboxes.empty()) c = cv::Point2f((bboxes[0].xyxy[0] + bboxes[0].xyxy[2]) / 2, (bboxes[0].xyxy[1] + bboxes[0].xyxy[3]) / 2);
  const cv::Point tl = engine.set_window_center(c);
  bboxes = engine.detect();
  const auto w1 = engine.window();
  engine.set_window(cv::Point(0, 0));
  const cv::Mat & rotated = engine.get_rotated_image();
  irmv_detection::IrmDetectorCore::Params params;
  params.window_size = cv::Size(640, 512);
  std::printf("src_bytes %zu centred %d %d moved %d %d == %d %d size %d x %d rotated %d x %d has_window %d params %d\n", engine.src_image_bytes(),
              w0.first.x, w0.first.y, tl.x, tl.y, w1.first.x, w1.first.y, w1.second.width, w1.second.height, rotated.cols, rotated.rows,
              engine.has_window() ? 1 : 0, params.window_size.width);
  return 0;
}
"""


def facade_exe():
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    os.makedirs(bindir, exist_ok=True)
    src = os.path.join(bindir, "window_facade_test.cpp")
    with open(src, "w") as f:
        f.write(FACADE_SRC)
    exe = os.path.join(bindir, "window_facade_test")
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_reference_style_window_code_compiles_against_the_facade():
    assert os.path.exists(facade_exe())
