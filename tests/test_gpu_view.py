"""Search view on the GPU: a slot of a window engine in the frame view is, bit for bit, a slot of a PLAIN engine -- no window,
the same full frame, net, blob and camera (P below) -- and in the window view it stays what tests/test_gpu_window.py says it
is: the plain engine of the window's size on the numpy crop, camera shifted by the corner.  No tolerances anywhere.

Geometries (all into a 128 x 64 net; tests/test_view.py asserts the front paths through irmv_front_plan):
  322 x 201 frame, 256 x 128 window: the frame view's front runs as three layers (width not a multiple of 4), the window
                                     view's fused, direct, on 8-row tiles;
  256 x 128 frame, 128 x  64 window: frame view fused and direct, window view fused and staged (1 : 1);
  320 x 200 frame, 128 x  64 window: both fused and staged, at different ratios.
The blob is test_gpu_window.py's crafted one: every compared case asserts a detection with a solved pose.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import test_gpu_window as tw
from irmv_detection_amd import bayer, capi, window
from irmv_detection_amd.engine import YoloEngine

pytestmark = pytest.mark.gpu

NET = (128, 64)
K = tw.K
GEOMETRIES = [((322, 201), (256, 128)), ((256, 128), (128, 64)), ((320, 200), (128, 64))]
FULL, WIN = GEOMETRIES[0]
CENTRE = ((FULL[0] - WIN[0]) // 2, (FULL[1] - WIN[1]) // 2)      # where every slot's window lies at creation


@pytest.fixture(scope="module")
def wblob(blob):
    return dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))


def plain(blob, full=FULL, net=NET, **kw):
    """P: the engine without a window on the full frame."""
    kw.setdefault("camera_matrix", K)
    return YoloEngine(None, full, weights_blob=blob, net_size=net[0], net_height=net[1], **kw)


_refs = {}


def p_refs(blob, idx, full=FULL, rot=True, tensors=True, **kw):
    """P's snapshots of synthetic frames idx on the full frame: one engine per case, computed once and shared."""
    key = ("P", full, rot, tuple(sorted(kw.items())))
    missing = [i for i in idx if (key, i) not in _refs]
    if missing:
        with plain(blob, full, rotate180=rot, **kw) as p:
            for i in missing:
                p.get_src_image_buffer()[:] = tw.frame_of(i, full)
                p.detect()
                _refs[(key, i)] = tw.snapshot(p, 0)
    return [_refs[(key, i)] for i in idx]


def w_refs(blob, idx, org=CENTRE, full=FULL, win=WIN, rot=True):
    """The window view's reference: the plain engine of the window's size on the crop at org, camera shifted by org."""
    key = ("W", full, win, rot, org)
    missing = [i for i in idx if (key, i) not in _refs]
    if missing:
        with tw.peng(blob, win, NET, org, rotate180=rot) as p:
            for i in missing:
                p.get_src_image_buffer()[:] = window.crop(tw.frame_of(i, full), org[0], org[1], win[0], win[1], rot)
                p.detect()
                _refs[(key, i)] = tw.snapshot(p, 0)
    return [_refs[(key, i)] for i in idx]


def same(got, ref, org=(0, 0), where=""):
    if "input" in got:
        tw.same_tensors(got, ref)
    n = tw.same_results(got, ref, org, where)
    assert n > 0, where
    return n


# ---- 1. frame view is the plain engine -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("full,win", GEOMETRIES)
def test_frame_view_is_the_plain_engine(wblob, full, win, rot):
    ref, = p_refs(wblob, [5], full, rot)
    with tw.weng(wblob, full, win, rotate180=rot) as w:
        assert w.view() == ("window", win)
        w.get_src_image_buffer()[:] = tw.frame_of(5, full)
        w.set_view("frame")
        assert w.view() == ("frame", full)
        w.detect()
        same(tw.snapshot(w, 0), ref, where=(full, win, rot))


# ---- 2. back and forth -----------------------------------------------------------------------------------------------------------
def test_back_and_forth_captures_each_graph_once(wblob, monkeypatch):
    monkeypatch.setenv("IRMV_SYNC_LAUNCH", "graph")
    rf, = p_refs(wblob, [3])
    rw, = w_refs(wblob, [3])
    with tw.weng(wblob) as w:
        assert w.sync_launch == "graph"
        w.get_src_image_buffer()[:] = tw.frame_of(3)
        counts = []
        for pair in range(2):
            w.set_view("window")
            w.detect()
            same(tw.snapshot(w, 0), rw, CENTRE, ("W", pair))
            w.set_view("frame")
            # results read after a later set_view still carry the view they were submitted in
            same(tw.snapshot(w, 0, False), rw, CENTRE, ("W after the switch", pair))
            w.detect()
            same(tw.snapshot(w, 0), rf, where=("F", pair))
            counts.append(w.debug_graph_count())
        assert counts[0] == counts[1] and counts[0] >= 2
        w.set_view("window")
        same(tw.snapshot(w, 0, False), rf, where="F after the switch")
        # a set_view between two asynchronous submits of one slot leaves the first with the old view
        w.submit(0, 1, async_upload=True)
        w.set_view("frame")                             # waits for the step in flight, then switches
        assert w.view()[0] == "frame"
        same(tw.snapshot(w, 0, False), rw, CENTRE, "in flight")
        w.submit(0, 1, async_upload=True)
        w.wait_slots(0, 1)
        same(tw.snapshot(w, 0, False), rf, where="switched")


# ---- 3. every launch form ----------------------------------------------------------------------------------------------------------
def test_every_launch_form_gives_the_same_bits(wblob, monkeypatch):
    idx = [40 + s for s in range(8)]
    fr = [tw.frame_of(i) for i in idx]
    rf, rw = p_refs(wblob, idx), w_refs(wblob, idx)
    forms = set()
    for mode in ("graph", "eager"):
        for wu in ("1", "0"):
            monkeypatch.setenv("IRMV_SYNC_LAUNCH", mode)
            monkeypatch.setenv("IRMV_WINDOW_UPLOAD", wu)
            whole = (mode, wu) == ("graph", "1")
            S = 8 if whole else 2
            with tw.weng(wblob, num_slots=S, num_streams=2) as w:
                assert w.sync_launch == mode
                for s in range(S):
                    w.get_src_image_buffer(s)[:] = fr[s]
                for view, refs, org in (("frame", rf, (0, 0)), ("window", rw, CENTRE), ("frame", rf, (0, 0))):
                    for s in range(S):
                        w.set_view(view, slot=s)
                        w.detect(s)
                        same(tw.snapshot(w, s, s == 0), refs[s], org, (mode, wu, view, s))
                forms.add(("detect", mode, wu))
                if not whole:
                    continue
                # batched: eight slots on two streams, all in the frame view, whole-frame uploads inside the graphs
                for s in range(8):
                    w.get_src_image_buffer(s)[:] = fr[7 - s]
                w.submit(0, 8)
                w.wait()
                for s in range(8):
                    same(tw.snapshot(w, s, False), rf[7 - s], where=("batched", s))
                forms.add("batched")
                # eight single-slot ASYNC_UPLOAD submits in flight: even slots in the window view (band copies), odd slots in
                # the frame view (whole frames)
                for s in range(8):
                    w.get_src_image_buffer(s)[:] = fr[(s + 3) % 8]
                    w.set_view("frame" if s % 2 else "window", slot=s)
                for s in range(8):
                    w.submit(s, 1, async_upload=True)
                for s in range(8):
                    w.wait_slots(s, 1)
                for s in range(8):
                    k = (s + 3) % 8
                    same(tw.snapshot(w, s, False), rf[k] if s % 2 else rw[k], (0, 0) if s % 2 else CENTRE, ("async", s))
                w.wait()
                forms.add("async")
                # a device-resident producer: frames written into the device slots, submitted without H2D
                for s in range(8):
                    w.set_view("frame", slot=s)
                    w.get_src_image_buffer(s)[:] = 0
                    tw._hip_memcpy_h2d(w.src_device_ptr(s), fr[s])
                w.submit(0, 8, h2d=False)
                w.wait()
                for s in range(8):
                    same(tw.snapshot(w, s, False), rf[s], where=("device", s))
                forms.add("device")
                # the stale band: a band upload in the window view, then another frame in the pinned slot and the frame view --
                # the rows outside the old band are the new frame's only if the upload follows the view
                w.set_view("window", slot=0)
                w.get_src_image_buffer(0)[:] = fr[1]
                w.submit(0, 1, async_upload=True)
                w.wait_slots(0, 1)
                same(tw.snapshot(w, 0, False), rw[1], CENTRE, "band")
                w.get_src_image_buffer(0)[:] = fr[6]
                w.set_view("frame", slot=0)
                w.submit(0, 1, async_upload=True)
                w.wait_slots(0, 1)
                same(tw.snapshot(w, 0), rf[6], where="stale band")
                forms.add("stale band")
    assert len(forms) == 8


# ---- 4. mixed group ------------------------------------------------------------------------------------------------------------------
def test_a_group_of_mixed_views_is_refused_before_anything_runs(wblob):
    rf = p_refs(wblob, [3, 11])
    rw, = w_refs(wblob, [3])
    with tw.weng(wblob, num_slots=2, num_streams=1) as w:
        for s, i in enumerate((3, 11)):
            w.get_src_image_buffer(s)[:] = tw.frame_of(i)
        w.detect(0)
        w.set_view("frame", slot=1)
        w.detect(1)
        rc = w._L.irmv_engine_submit(w._h, 0, 2, capi.SUBMIT_H2D)
        msg = w._L.irmv_last_error()
        assert rc == capi.ERR_ARG and b"slots 0 and 1" in msg and b"view" in msg, msg
        same(tw.snapshot(w, 0, False), rw, CENTRE, "slot 0 kept its results")
        same(tw.snapshot(w, 1, False), rf[1], where="slot 1 kept its results")
        w.set_view("frame", slot=0)
        w.submit(0, 2)
        w.wait()
        for s in range(2):
            same(tw.snapshot(w, s, False), rf[s], where=("one view", s))


# ---- 5. Bayer --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bilinear", "mhc"])
def test_bayer_frame_view_is_the_plain_bayer_engine(wblob, algo):
    full, pattern = (322, 202), "GRBG"
    raw = bayer.mosaic(tw.frame_of(5, full), pattern)
    gains, lut = (300, 256, 420), (255 - np.arange(256)).astype(np.uint8)
    kw = dict(src_format=pattern, bayer_demosaic=algo)
    with tw.weng(wblob, full=full, **kw) as w, plain(wblob, full, **kw) as p:
        w.set_view("frame")
        for e in (w, p):
            e.get_src_image_buffer()[:] = raw
        for isp in (False, True):
            for e in (w, p):
                if isp:
                    e.set_bayer_isp(gains, lut)
                e.detect()
            same(tw.snapshot(w, 0), tw.snapshot(p, 0), where=(algo, isp))
        hwc = bayer.demosaic(raw, pattern, gains, algo, lut)
        assert np.array_equal(w.get_rotated_image(), hwc[::-1, ::-1])


# ---- 6. classical points ---------------------------------------------------------------------------------------------------------------
def test_classical_points_in_the_frame_view(blob, rm_test_image):
    """rm_test.jpg at the sizes of test_gpu_window.py's classical case; the blob's Detect finals are crafted as there."""
    full, win, net, rot = (1280, 1024), (640, 512), (640, 512), False
    lit = {0: ("bias", dc.dark_bias(14)), 1: ("bias", dc.dark_bias(14)), 2: ("bias", dc.two_tied_bias(14))}
    b = dc.craft(blob, cls=lit, box=("bias", dc.dfl_bias(3)))
    kw = dict(point_source=capi.POINTS_CLASSICAL, rotate180=rot, armor_size=capi.ARMOR_LARGE)
    with tw.weng(b, full, win, net, **kw) as w, plain(b, full, net, **kw) as p:
        w.set_view("frame")
        for e in (w, p):
            e.get_src_image_buffer()[:] = rm_test_image
            e.detect()
        got, ref = tw.snapshot(w, 0, False), tw.snapshot(p, 0, False)
        same(got, ref, where="in step")
        assert any(d["ints"][3] == 1 and d["ints"][5] == 2 for d in got["dets"])
        boxes = np.array([[630, 360, 785, 420], [600, 340, 820, 440], [500, 300, 900, 500], [630, 360, 700, 420], [420, 160, 1030, 650],
                          [100, 100, 300, 300]], np.float32)
        ga, ra = w.extract_armors_raw(boxes), p.extract_armors_raw(boxes)
        n = 0
        for i in range(len(boxes)):
            assert bytes(ga[i]) == bytes(ra[i]), i
            n += ga[i].pnp_ok
        assert n >= 3
        rotated = w.get_rotated_image()
        assert rotated.shape == (1024, 1280, 3) and np.array_equal(rotated, rm_test_image[::-1, ::-1])
        w.set_view("window")
        assert w.get_rotated_image().shape == (512, 640, 3)


# ---- 7. profile --------------------------------------------------------------------------------------------------------------------------
def test_profile_follows_the_view(wblob, monkeypatch):
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_HEAD", "0")
    with plain(wblob, num_slots=2) as p:
        whole = {c: [k["name"] for k in p.profile(0, c)] for c in (1, 2)}
    with tw.peng(wblob, num_slots=2) as p:
        crop = {c: [k["name"] for k in p.profile(0, c)] for c in (1, 2)}
    assert "front_fused" in crop[1] and "front_fused" not in whole[1] and "preprocess" in whole[1]
    with tw.weng(wblob, num_slots=2) as w:
        for c in (1, 2):
            assert [k["name"] for k in w.profile(0, c)] == ["window_crop"] + crop[c]
        for s in range(2):
            w.set_view("frame", slot=s)
        for c in (1, 2):
            names = [k["name"] for k in w.profile(0, c)]
            assert names == whole[c] and "window_crop" not in names
        w.set_view("window", slot=0)
        assert [k["name"] for k in w.profile(0, 1)] == ["window_crop"] + crop[1]     # what it is today
        with pytest.raises(capi.IrmvError):
            w.profile(0, 2)                                                         # slots 0 and 1 in different views


# ---- 8. window state across views ----------------------------------------------------------------------------------------------------------
def test_set_window_in_the_frame_view_waits_for_the_window_view(wblob):
    org = (3, 70)
    rf, = p_refs(wblob, [11])
    rw, = w_refs(wblob, [11], org)
    with tw.weng(wblob) as w:
        w.get_src_image_buffer()[:] = tw.frame_of(11)
        w.set_view("frame")
        w.detect()
        same(tw.snapshot(w, 0, False), rf, where="before")
        w.set_window(*org)
        assert w.window() == (org[0], org[1], WIN[0], WIN[1]) and w.view() == ("frame", FULL)
        w.detect()
        same(tw.snapshot(w, 0), rf, where="the corner moved, the frame view did not")
        w.set_view("window")
        assert w.window() == (org[0], org[1], WIN[0], WIN[1])
        w.detect()
        same(tw.snapshot(w, 0), rw, org, "back in the window")


# ---- 9. errors on a live engine --------------------------------------------------------------------------------------------------------------
def test_errors_on_a_live_engine(wblob):
    rf, = p_refs(wblob, [5])
    with plain(wblob) as p:
        assert p._L.irmv_engine_set_view(p._h, 0, capi.VIEW_FRAME) == capi.ERR_ARG and b"no window" in p._L.irmv_last_error()
        assert p._L.irmv_engine_set_view(p._h, 0, capi.VIEW_WINDOW) == capi.ERR_ARG
        assert p._L.irmv_engine_get_view(p._h, 0, None, None, None) == capi.ERR_ARG
        p.get_src_image_buffer()[:] = tw.frame_of(5)
        p.detect()
        same(tw.snapshot(p, 0, False), rf, where="plain engine afterwards")
    with tw.weng(wblob, num_slots=2) as w:
        L, h = w._L, w._h
        for slot in (-1, 2):
            assert L.irmv_engine_set_view(h, slot, capi.VIEW_FRAME) == capi.ERR_ARG and b"slot" in L.irmv_last_error()
            assert L.irmv_engine_get_view(h, slot, None, None, None) == capi.ERR_ARG
        for view in (2, -1):
            assert L.irmv_engine_set_view(h, 0, view) == capi.ERR_ARG and b"view" in L.irmv_last_error()
        assert w.view(0) == ("window", WIN) and w.view(1) == ("window", WIN)       # the refused calls changed nothing
        v = C.c_int(-1)
        assert L.irmv_engine_get_view(h, 1, C.byref(v), None, None) == capi.OK and v.value == capi.VIEW_WINDOW
        w.get_src_image_buffer()[:] = tw.frame_of(5)
        w.set_view("frame")
        w.detect()
        same(tw.snapshot(w, 0, False), rf, where="window engine afterwards")
    # a frame whose letterboxed image would have no row: the window passes irmv_engine_create, the frame view is refused
    with tw.weng(wblob, full=(4000, 14), win=(40, 14), resize_mode=capi.RESIZE_LETTERBOX) as w:
        assert w._L.irmv_engine_set_view(w._h, 0, capi.VIEW_FRAME) == capi.ERR_ARG and b"letterbox" in w._L.irmv_last_error()
        assert w.view() == ("window", (40, 14))
        w.detect()
