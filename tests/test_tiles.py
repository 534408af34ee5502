"""Tiled search on the host: the grid irmv_tile_grid documents against irmv_detection_amd.tiles.grid, the merge reference on
hand-written lists whose answers are stated here, and the irmv_tile_det record against its ctypes mirror.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from irmv_detection_amd import _build, capi, tiles


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


# ---- grid ------------------------------------------------------------------------------------------------------------------
def test_worked_examples(lib):
    c, nx, ny = capi.tile_grid((1280, 1024), (640, 512), 128)
    assert (nx, ny) == (3, 3) and c == [(x, y) for y in (0, 256, 512) for x in (0, 320, 640)]
    c, nx, ny = capi.tile_grid((320, 200), (128, 64), (32, 16))
    assert (nx, ny) == (3, 4) and c == [(x, y) for y in (0, 45, 91, 136) for x in (0, 96, 192)]
    assert tiles.grid((1280, 1024), (640, 512), 128) == capi.tile_grid((1280, 1024), (640, 512), 128)
    assert tiles.grid((320, 200), (128, 64), (32, 16)) == capi.tile_grid((320, 200), (128, 64), (32, 16))


SWEEP = [((1280, 1024), (640, 512)), ((322, 201), (256, 128)), ((320, 200), (128, 64)), ((640, 512), (640, 512)),
         ((1280, 1024), (640, 1024)), ((1000, 700), (384, 320)), ((641, 513), (640, 512)), ((2048, 1536), (640, 512))]


def test_grid_equals_the_reference_and_covers_the_frame(lib):
    checked = refused = 0
    for frame, win in SWEEP:
        for ox in (0, 1, 17, win[0] // 4, win[0] // 2, win[0] - 1):
            for oy in (0, 16, win[1] // 3, win[1] - 1):
                try:
                    ref = tiles.grid(frame, win, (ox, oy))
                except ValueError:
                    with pytest.raises(capi.IrmvError):
                        capi.tile_grid(frame, win, (ox, oy))
                    refused += 1
                    continue
                got = capi.tile_grid(frame, win, (ox, oy))
                assert got == ref, (frame, win, ox, oy)
                corners, nx, ny = got
                assert len(corners) == nx * ny <= capi.MAX_TILES
                for (F, w, ov, cs) in ((frame[0], win[0], ox, [corners[i][0] for i in range(nx)]),
                                       (frame[1], win[1], oy, [corners[i * nx][1] for i in range(ny)])):
                    assert cs[0] == 0 and cs[-1] == F - w                          # every pixel from the first to the last ...
                    assert all(0 <= c <= F - w for c in cs)                        # corners inside the frame
                    assert all(b > a for a, b in zip(cs, cs[1:]))
                    assert all(a + w - b >= ov for a, b in zip(cs, cs[1:]))        # ... is covered; neighbours overlap by >= ov
                    covered = np.zeros(F, bool)
                    for c in cs:
                        covered[c:c + w] = True
                    assert covered.all()
                    if len(cs) > 1:                                                # the fewest tiles: one fewer cannot do it
                        assert (len(cs) - 1) * (w - ov) + ov < F
                checked += 1
    assert checked > 100 and refused > 0


def test_grid_refusals(lib):
    cfg = capi._geometry_cfg((1280, 1024), 640, 512, capi.RESIZE_STRETCH, True, capi.SRC_HWC8, None)
    n, nx, ny = C.c_int(0), C.c_int(0), C.c_int(0)
    L = lib
    assert L.irmv_tile_grid(C.byref(cfg), 0, 0, None, 0, C.byref(n), None, None) == capi.ERR_ARG and b"no window" in L.irmv_last_error()
    cfg = capi._geometry_cfg((1280, 1024), 640, 512, capi.RESIZE_STRETCH, True, capi.SRC_HWC8, (640, 512))
    assert L.irmv_tile_grid(C.byref(cfg), 0, 0, None, 0, None, None, None) == capi.ERR_ARG
    assert L.irmv_tile_grid(None, 0, 0, None, 0, C.byref(n), None, None) == capi.ERR_ARG
    for ox, oy in [(-1, 0), (0, -1), (640, 0), (0, 512)]:
        assert L.irmv_tile_grid(C.byref(cfg), ox, oy, None, 0, C.byref(n), None, None) == capi.ERR_ARG and b"overlap" in L.irmv_last_error()
    assert L.irmv_tile_grid(C.byref(cfg), 600, 0, None, 0, C.byref(n), None, None) == capi.ERR_ARG and b"IRMV_MAX_TILES" in L.irmv_last_error()   # 17 x 2
    assert L.irmv_tile_grid(C.byref(cfg), 639, 511, None, 0, C.byref(n), None, None) == capi.ERR_ARG                                          # 641 x 513
    assert L.irmv_tile_grid(C.byref(cfg), 128, 128, None, 0, C.byref(n), C.byref(nx), C.byref(ny)) == capi.OK and (n.value, nx.value, ny.value) == (9, 3, 3)
    xy = (C.c_int32 * 18)()
    assert L.irmv_tile_grid(C.byref(cfg), 128, 128, xy, 8, C.byref(n), None, None) == capi.ERR_ARG and b"cap" in L.irmv_last_error()
    assert L.irmv_tile_grid(C.byref(cfg), 128, 128, xy, 9, C.byref(n), None, None) == capi.OK and list(xy)[-2:] == [640, 512]
    with pytest.raises(ValueError):
        tiles.grid((1280, 1024), (640, 512), 640)
    with pytest.raises(ValueError):
        tiles.grid((1280, 1024), (640, 512), (600, 0))


# ---- merge reference ---------------------------------------------------------------------------------------------------------
FRAME, WIN = (300, 100), (200, 100)          # two tiles side by side: columns [0, 200) and [100, 300); the seam band is [100, 200)
CORNERS = [(0, 0), (100, 0)]


def L(*recs):
    """recs: (x1, y1, x2, y2, score, cls)"""
    a = np.array(recs, np.float32).reshape(-1, 6)
    return dict(boxes=a[:, :4].copy(), scores=a[:, 4].copy(), classes=a[:, 5].astype(int))


def run(lists, corners=CORNERS, **kw):
    return tiles.merge(lists, corners, WIN, FRAME, **kw)


def by_id(trace):
    return {(t["tile"], t["index"]): t for t in trace}


def test_cross_tile_duplicate():
    """Both tiles see the whole armor in the overlap: the higher score stays, the other tile's copy goes."""
    kept, trace = run([L((120, 20, 160, 40, 0.80, 3)), L((121, 20, 161, 40, 0.90, 3))])
    assert kept == [(1, 0, 0)]
    t = by_id(trace)
    assert t[(0, 0)]["rule"] == "suppressed" and t[(0, 0)]["by"] == (1, 0) and t[(1, 0)]["rule"] == "kept"


def test_seam_cut_partial_box_loses_to_a_lower_scored_whole_box():
    """Tile 0 sees the armor cut off at its right edge (x2 = 199.5 > 200 - 2) with the higher score; tile 1 sees it whole."""
    kept, trace = run([L((170, 20, 199.5, 40, 0.95, 5)), L((170, 20, 215, 40, 0.60, 5))])
    assert kept == [(1, 0, 0)]
    t = by_id(trace)
    assert t[(0, 0)]["cut"] == 1 and t[(0, 0)]["rule"] == "suppressed" and t[(0, 0)]["by"] == (1, 0) and t[(0, 0)]["score"] > t[(1, 0)]["score"]
    assert [(r["tile"], r["index"]) for r in trace] == [(1, 0), (0, 0)]           # whole boxes first, whatever the score
    # the frame's own edges cut nothing: the same box at the frame's left edge and the tile-0 box at x1 = 0
    kept, trace = run([L((0, 20, 30, 40, 0.9, 5)), L((270, 20, 300, 40, 0.9, 5))])
    assert kept == [(0, 0, 0), (1, 0, 0)]
    # a cut box nothing whole covers is kept, flagged
    kept, _ = run([L((170, 20, 199.5, 40, 0.95, 5)), L()])
    assert kept == [(0, 0, 1)]
    # the margin decides: 197.9 is inside it, 198.0 is not (x2 > 200 - 2 is false)
    assert list(tiles.cut_flags([[150, 20, 198.0, 40], [150, 20, 198.5, 40]], (0, 0), WIN, FRAME, 2.0)) == [False, True]
    assert list(tiles.cut_flags([[101.9, 20, 150, 40], [102.0, 20, 150, 40]], (100, 0), WIN, FRAME, 2.0)) == [True, False]


def test_overlapping_boxes_of_different_classes_are_both_kept():
    kept, trace = run([L((120, 20, 160, 40, 0.80, 3)), L((120, 20, 160, 40, 0.90, 4))])
    assert kept == [(1, 0, 0), (0, 0, 0)]
    assert by_id(trace)[(0, 0)]["spared_other_class"] == [(1, 0)]


def test_same_tile_nested_pair_is_kept():
    """Their own NMS let both through (IoU below its threshold; intersection over the smaller is 1): the merge does not rule again."""
    kept, trace = run([L((110, 10, 190, 90, 0.90, 2), (130, 30, 150, 50, 0.70, 2)), L()])
    assert kept == [(0, 0, 0), (0, 1, 0)]
    assert by_id(trace)[(0, 1)]["spared_same_tile"] == [(0, 0)]
    # ... while the same small box from the other tile goes
    kept, _ = run([L((110, 10, 190, 90, 0.90, 2)), L((130, 30, 150, 50, 0.70, 2))])
    assert kept == [(0, 0, 0)]


def test_exact_score_tie_across_tiles_goes_to_the_lower_tile():
    kept, trace = run([L((120, 20, 160, 40, 0.75, 1)), L((120, 20, 160, 40, 0.75, 1))])
    assert kept == [(0, 0, 0)] and by_id(trace)[(1, 0)]["by"] == (0, 0)
    kept, _ = run([L((120, 20, 160, 40, 0.75, 1), (120, 60, 160, 80, 0.75, 1)), L()])                # ... then to the lower index
    assert kept == [(0, 0, 0), (0, 1, 0)]


def test_max_det_cap_and_empty_tiles():
    many = [(105 + 8 * i, 10, 111 + 8 * i, 20, 0.9 - 0.01 * i, 0) for i in range(10)]
    kept, trace = run([L(), L(*many)], max_det=4)
    assert kept == [(1, i, 0) for i in range(4)]
    assert [t["rule"] for t in trace] == ["kept"] * 4 + ["cap"] * 6
    assert run([L(), L()]) == ([], [])
    kept, _ = run([L(), L(), L((150, 5, 170, 20, 0.5, 0))], corners=[(0, 0), (50, 0), (100, 0)])
    assert kept == [(2, 0, 0)]


def test_ios_is_intersection_over_the_smaller_area_without_division():
    a, b = np.array([0, 0, 10, 10], np.float32), np.array([5, 0, 25, 10], np.float32)   # inter 50, areas 100 and 200
    assert tiles.ios_gt(a, b, 0.49) and not tiles.ios_gt(a, b, 0.5) and not tiles.ios_gt(a, b, 0.51)
    assert not tiles.ios_gt(a, np.array([10, 0, 20, 10], np.float32), 0.01)            # touching: inter 0 > 0 is false
    kept, _ = run([L((120, 20, 160, 40, 0.80, 3)), L((140, 20, 180, 40, 0.90, 3))])    # inter = half of either: not > 0.5 x
    assert kept == [(1, 0, 0), (0, 0, 0)]
    kept, _ = run([L((120, 20, 160, 40, 0.80, 3)), L((140, 20, 180, 40, 0.90, 3))], ios_thr=0.49)
    assert kept == [(1, 0, 0)]


# ---- record layout ------------------------------------------------------------------------------------------------------------
def test_tile_det_record_matches_the_header(tmp_path):
    fields = [f for f, _ in capi.TileDet._fields_]
    src = tmp_path / "td.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %d", sizeof(irmv_tile_det), IRMV_MAX_TILES);' +
                   "".join(f'printf(" %zu", offsetof(irmv_tile_det, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "td"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.TileDet), capi.MAX_TILES] + [getattr(capi.TileDet, f).offset for f in fields]
    assert C.sizeof(capi.TileDet) == C.sizeof(capi.Det) + 16 and tiles.MAX_TILES == capi.MAX_TILES


# ---- C++ facade ------------------------------------------------------------------------------------------------------------------
def facade_exe(build=True):
    """tests/cpp/tiles_facade_test.cpp against the facade headers (built here so that the binary travels to the GPU box with the tree)."""
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    exe = os.path.join(bindir, "tiles_facade_test")
    if build or not os.path.exists(exe):
        os.makedirs(bindir, exist_ok=True)
        _build.build()
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "tiles_facade_test.cpp"), "-o", exe,
                               "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_lost_target_loop_compiles_against_the_facade():
    assert os.path.exists(facade_exe())
