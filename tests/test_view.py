"""Search view, host side: the three new symbols and their constants, the front plans that make the two views of the test
geometries take different paths, the Python mirror's argument check, and the C++ facade.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from irmv_detection_amd import _build, capi
from irmv_detection_amd.engine import YoloEngine

NET = (128, 64)
# (full frame, window): tests/test_gpu_view.py runs these
GEOMETRIES = [((322, 201), (256, 128)), ((256, 128), (128, 64)), ((320, 200), (128, 64))]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def test_the_new_symbols_are_bound_and_the_constants_match_the_header(lib):
    names = [s[0] for s in capi.SYMBOLS]
    for sym in ("irmv_engine_set_view", "irmv_engine_get_view", "irmv_engine_debug_graph_count"):
        assert sym in names and hasattr(lib, sym)
    header = open(os.path.join(ROOT, "include", "irmv_hip.h")).read()
    consts = dict(re.findall(r"#define\s+(IRMV_VIEW_\w+)\s+(\d+)", header))
    assert consts == {"IRMV_VIEW_WINDOW": str(capi.VIEW_WINDOW), "IRMV_VIEW_FRAME": str(capi.VIEW_FRAME)}
    assert capi.VIEWS == {"window": capi.VIEW_WINDOW, "frame": capi.VIEW_FRAME} and capi.VIEW_WINDOW != capi.VIEW_FRAME
    # the configuration struct did not grow
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(capi.EngineCfg) and capi.EngineCfg.win_height.offset + 2 == C.sizeof(capi.EngineCfg)


def test_null_engines_are_refused(lib):
    assert lib.irmv_engine_set_view(None, 0, capi.VIEW_FRAME) == capi.ERR_ARG
    assert lib.irmv_engine_get_view(None, 0, None, None, None) == capi.ERR_ARG
    assert lib.irmv_engine_debug_graph_count(None) == 0


@pytest.mark.parametrize("rot", [True, False])
def test_the_two_views_of_the_test_geometries_reach_different_front_paths(lib, rot):
    """The frame view's plan is irmv_front_plan's for the same configuration with win_* = 0."""
    plan = lambda size, win=None: capi.front_plan(size, NET[0], NET[1], capi.RESIZE_STRETCH, rot, window=win)
    # 322 x 201: a pitch of 966 bytes and a frame of 194,166 bytes, neither a multiple of 16
    assert (322 * 3) % 16 != 0 and (322 * 201 * 3) % 16 != 0
    f, w = plan((322, 201)), plan((322, 201), (256, 128))
    assert not f["fused"] and f["reason"] == capi.FRONT_WIDTH_MOD4
    assert w["fused"] and w["fastx"] == 3 and w["tile_y"] == 8
    f, w = plan((256, 128)), plan((256, 128), (128, 64))
    assert f["fused"] and f["fastx"] == 3 and f["tile_y"] == 8
    assert w["fused"] and w["fastx"] == 0                       # 1 : 1, staged
    f, w = plan((320, 200)), plan((320, 200), (128, 64))
    assert f["fused"] and f["fastx"] == 0                       # 2.5 : 1 and 3.125 : 1, staged
    assert w["fused"] and w["fastx"] == 0
    for full, win in GEOMETRIES:
        assert plan(full, win) == plan(win)                     # the window view: the plan of the window-sized source


def test_the_python_mirror_rejects_an_unknown_view_name_before_calling_the_library():
    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")

    e = YoloEngine.__new__(YoloEngine)
    e._L, e._h, e.slot = Lib(), None, 0
    for bad in ("full", "Frame", "", None, 1):
        with pytest.raises(ValueError):
            e.set_view(bad)


FACADE_SRC = r"""
#include <cstdio>
#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/yolo_engine.hpp"

using irmv_detection::YoloEngine;

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  YoloEngine engine(argv[1], cv::Size(1280, 1024), true, -1, false, 640, IRMV_SRC_HWC8, {256, 256, 256}, 512,
                    IRMV_DEMOSAIC_BILINEAR, cv::Size(640, 512));
  engine.set_view(YoloEngine::View::Frame);      // at start-up: the frame view is built here, not on the first lost target
  engine.set_view(YoloEngine::View::Window);
  int searched = 0;
  for (int frame = 0; frame < 4; frame++) {
    // (the producer has written the frame into engine.get_src_image_buffer())
    auto bboxes = engine.detect();
    if (bboxes.empty() && engine.view() == YoloEngine::View::Window) {
      engine.set_view(YoloEngine::View::Frame);  // lost: the same pinned frame again, on the whole frame
      bboxes = engine.detect();
      searched++;
    }
    if (!bboxes.empty()) {
      engine.set_window_center(cv::Point2f((bboxes[0].xyxy[0] + bboxes[0].xyxy[2]) / 2, (bboxes[0].xyxy[1] + bboxes[0].xyxy[3]) / 2));
      engine.set_view(YoloEngine::View::Window);
    }
  }
  const cv::Mat & rotated = engine.get_rotated_image();
  std::printf("view %d searched %d rotated %d x %d\n", engine.view() == YoloEngine::View::Frame ? 1 : 0, searched, rotated.cols, rotated.rows);
  return 0;
}
"""


def test_reference_style_view_code_compiles_against_the_facade():
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    os.makedirs(bindir, exist_ok=True)
    src = os.path.join(bindir, "view_facade_test.cpp")
    with open(src, "w") as f:
        f.write(FACADE_SRC)
    exe = os.path.join(bindir, "view_facade_test")
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    assert os.path.exists(exe)
