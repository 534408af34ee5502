"""Debug images on the GPU (irmv_engine_render, csrc/k_render.hip): every picture equals, byte for byte, the host reference
irmv_detection_amd/render.py applied to the frame the engine itself hands out -- get_rotated_image(), or with rotate180 = 0 the
frame as stored.  One-slot engines at a 64 x 64 net:

  hwc       100 x 68 HWC, rotate180 1 and 0
  odd       101 x 67: the dropped column and row at scales 2 and 4, rows of 303 bytes that no store width divides
  bayer     100 x 68 RGGB after set_bayer_isp with non-identity gains and tone LUT
  window    160 x 128 with a 100 x 68 window at corner (13, 7), in the window view and in the frame view

The marks come from tests/render_zoo.py through explicit records; tests/test_render.py checks the reference itself.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
from irmv_detection_amd import capi, render
from irmv_detection_amd.engine import ArmorClass, YoloEngine, bbox
from render_zoo import shifted, stacked, zoo

pytestmark = pytest.mark.gpu

KINDS, SCALES = ("color", "binary"), (1, 2, 4)


@pytest.fixture(scope="module")
def cblob(blob):
    """Every anchor a candidate of two classes, an armor-like quad around it: detections with points on every frame."""
    return dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))


def frame_of(w, h, seed, channels=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, channels) if channels else (h, w), dtype=np.uint8)


def eng(blob, size, **kw):
    return YoloEngine(None, size, weights_blob=blob, net_size=64, **kw)


def to_dets(recs):
    out = []
    for r in recs:
        d = capi.Det()
        d.xyxy, d.kpts = (C.c_float * 4)(*r["xyxy"]), (C.c_float * 8)(*r["kpts"])
        d.class_id, d.armor_valid = r["class_id"], r["armor_valid"]
        out.append(d)
    return out


def check_pictures(e, R, recs, corner=(0, 0), thr=150, mark_sets=(7, 1, 2, 4)):
    """Both kinds at the three scales: without marks, and with the records under each set of mark bits."""
    dets = to_dets(recs)
    for kind in KINDS:
        for s in SCALES:
            assert e.render_dims(s) == render.dims(R.shape[1], R.shape[0], s)
            got = e.render(kind, s, 0, dets)
            assert got.shape == (R.shape[0] // s, R.shape[1] // s, 3)
            assert np.array_equal(got, render.render(R, kind, s, 0, (), corner, thr)), (kind, s, "no marks")
            for marks in mark_sets:
                exp = render.render(R, kind, s, marks, recs, corner, thr)
                assert np.array_equal(e.render(kind, s, marks, dets), exp), (kind, s, marks)
    assert np.array_equal(e.render("color", 1, 0, []), R)      # the rotated image itself


@pytest.fixture(scope="module")
def hwc(cblob):
    with eng(cblob, (100, 68)) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 1)
        yield e


def test_hwc_rotated(hwc):
    R = hwc.get_rotated_image()
    assert np.array_equal(R, frame_of(100, 68, 1)[::-1, ::-1])
    check_pictures(hwc, R, zoo(100, 68))


def test_hwc_as_stored(cblob):
    f = frame_of(100, 68, 2)
    with eng(cblob, (100, 68), rotate180=False) as e:
        e.get_src_image_buffer()[:] = f
        check_pictures(e, f, zoo(100, 68))


def test_odd_size_drops_a_column_and_a_row(cblob):
    with eng(cblob, (101, 67)) as e:
        e.get_src_image_buffer()[:] = frame_of(101, 67, 3)
        check_pictures(e, e.get_rotated_image(), zoo(101, 67))


def test_bayer_engine_renders_the_demosaiced_frame(cblob):
    lut = np.stack([np.clip(np.arange(256) * 1.3, 0, 255), 255 - np.arange(256), (np.arange(256) // 3) * 3]).astype(np.uint8)
    with eng(cblob, (100, 68), src_format="RGGB") as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 4, channels=0)
        plain = e.get_rotated_image()
        e.set_bayer_isp((300, 256, 200), lut)
        R = e.get_rotated_image()
        assert not np.array_equal(R, plain)
        check_pictures(e, R, zoo(100, 68), mark_sets=(7,))


def test_window_engine_in_both_views(cblob):
    with eng(cblob, (160, 128), window=(100, 68)) as e:
        e.get_src_image_buffer()[:] = frame_of(160, 128, 5)
        e.set_window(13, 7)
        full = frame_of(160, 128, 5)[::-1, ::-1]
        R = e.get_rotated_image()
        assert np.array_equal(R, full[7:75, 13:113])
        check_pictures(e, R, shifted(zoo(100, 68), 13, 7), corner=(13, 7), mark_sets=(7,))
        e.detect()
        own = e.results_raw()
        assert len(own) > 0
        assert np.array_equal(e.render("color", 2), e.render("color", 2, dets=own))
        assert np.array_equal(e.render("color", 2), render.render(R, "color", 2, 7, own, (13, 7)))
        e.set_view("frame")
        assert np.array_equal(e.get_rotated_image(), full)
        check_pictures(e, full, zoo(160, 128), mark_sets=(7,))
        e.detect()
        own = e.results_raw()
        assert len(own) > 0
        assert np.array_equal(e.render("binary", 1), render.render(full, "binary", 1, 7, own))
        e.set_view("window")
        assert np.array_equal(e.render("color", 1, 0, []), R)


def test_scale_one_boxes_and_labels_are_visualize_bboxes(hwc):
    recs = [r for r in zoo(100, 68) if all(render.coord(v, 0, 1) is not None for v in r["xyxy"])]
    exp = hwc.get_rotated_image()
    hwc.visualize_bboxes(exp, [bbox(r["xyxy"], 0.5, ArmorClass(r["class_id"] if 0 <= r["class_id"] < 14 else 14)) for r in recs])
    assert np.array_equal(hwc.render("color", 1, capi.MARK_BOXES | capi.MARK_LABELS, to_dets(recs)), exp)
    assert not np.array_equal(exp, hwc.get_rotated_image())


def test_last_results_graphs_and_records_are_left_alone(cblob):
    with eng(cblob, (100, 68)) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 6)
        R = e.get_rotated_image()
        # before the first detect(): whatever irmv_engine_results holds (creation times a step on slot 0's empty frame)
        assert np.array_equal(e.render("color", 1), e.render("color", 1, dets=e.results_raw()))
        e.detect()
        before = [bytes(d) for d in e.results_raw()]
        assert len(before) > 0 and any(d.armor_valid == 1 for d in e.results_raw())
        graphs = e.debug_graph_count()
        for kind in KINDS:
            for s in SCALES:
                own = e.render(kind, s)
                assert np.array_equal(own, e.render(kind, s, dets=e.results_raw()))
                assert np.array_equal(own, render.render(R, kind, s, 7, e.results_raw(), binary_threshold=150))
        assert not np.array_equal(e.render("color", 1), R)
        armors = e.results(0)                                                 # Armor objects draw what their records draw
        assert np.array_equal(e.render("color", 1, dets=armors), e.render("color", 1))
        assert e.debug_graph_count() == graphs
        assert [bytes(d) for d in e.results_raw()] == before
        e.detect()
        assert [bytes(d) for d in e.results_raw()] == before
        assert e.debug_graph_count() == graphs


def test_binary_threshold_follows_the_engine_and_the_opts_override_it(hwc):
    R = hwc.get_rotated_image()
    cd = (C.c_double * 4)(0.8, 3.2, 3.2, 5.5)
    try:
        assert np.array_equal(hwc.render("binary", 1, 0, []), render.render(R, "binary", 1, 0, (), binary_threshold=150))
        capi.check(hwc._L.irmv_engine_set_extract_params(hwc._h, 77, 0.1, 0.4, 40.0, cd))
        for s in SCALES:
            assert np.array_equal(hwc.render("binary", s, 0, []), render.render(R, "binary", s, 0, (), binary_threshold=77))
            assert np.array_equal(hwc.render("binary", s, 0, [], binary_threshold=200), render.render(R, "binary", s, 0, (), binary_threshold=200))
        for t in (0, 255):
            assert np.array_equal(hwc.render("binary", 1, 0, [], binary_threshold=t), render.render(R, "binary", 1, 0, (), binary_threshold=t))
        assert hwc.render("binary", 1, 0, [], binary_threshold=255).max() == 0
    finally:
        capi.check(hwc._L.irmv_engine_set_extract_params(hwc._h, 150, 0.1, 0.4, 40.0, cd))


def test_no_records_and_the_most_records_in_one_tile(cblob):
    with eng(cblob, (100, 68), max_det=256) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 7)
        R = e.get_rotated_image()
        recs = stacked(256)
        dets = to_dets(recs)
        for s in SCALES:
            assert np.array_equal(e.render("color", s, 7, []), render.render(R, "color", s))
            assert np.array_equal(e.render("color", s, 7, dets), render.render(R, "color", s, 7, recs)), s
        assert np.array_equal(e.render("binary", 1, 7, dets), render.render(R, "binary", 1, 7, recs))
        assert np.array_equal(e.render("color", 1, 7, dets[:255] + dets[:1]), render.render(R, "color", 1, 7, recs[:255] + recs[:1]))


def test_argument_errors_leave_the_engine_usable(hwc):
    L, h = hwc._L, hwc._h
    R = hwc.get_rotated_image()
    out = np.zeros((68, 100, 3), np.uint8)
    dst = out.ctypes.data_as(C.POINTER(C.c_uint8))
    dets = (capi.Det * hwc.max_det)()
    graphs = hwc.debug_graph_count()

    def opts(**kw):
        o = capi.render_opts(capi.RENDER_COLOR, 1, 7, -1)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    bad = [opts(struct_size=0), opts(struct_size=C.sizeof(capi.RenderOpts) + 4), opts(kind=2), opts(kind=-1), opts(scale=0), opts(scale=3),
           opts(scale=8), opts(marks=8), opts(marks=0x80000007), opts(reserved=0), opts(reserved=1), opts(reserved=2),
           opts(binary_threshold=-2), opts(binary_threshold=256)]
    for o in bad:
        assert L.irmv_engine_render(h, 0, C.byref(o), None, 0, dst) == capi.ERR_ARG
    good = opts()
    assert L.irmv_engine_render(h, 0, None, None, 0, dst) == capi.ERR_ARG
    assert L.irmv_engine_render(h, 0, C.byref(good), None, 0, None) == capi.ERR_ARG
    for slot in (-1, 1):
        assert L.irmv_engine_render(h, slot, C.byref(good), None, 0, dst) == capi.ERR_ARG
    for d, n in ((None, 1), (None, -2), (dets, -1), (dets, hwc.max_det + 1)):
        assert L.irmv_engine_render(h, 0, C.byref(good), d, n, dst) == capi.ERR_ARG
    w, hh = C.c_int(0), C.c_int(0)
    for slot, s in ((0, 3), (0, 0), (1, 1), (-1, 2)):
        assert L.irmv_engine_render_dims(h, slot, s, C.byref(w), C.byref(hh)) == capi.ERR_ARG
    assert L.irmv_engine_render_dims(h, 0, 1, None, C.byref(hh)) == capi.ERR_ARG
    assert (out == 0).all()
    assert L.irmv_engine_render(h, 0, C.byref(good), dets, 0, dst) == capi.OK and np.array_equal(out, R)
    assert hwc.debug_graph_count() == graphs
    check_pictures(hwc, R, zoo(100, 68)[:6], mark_sets=(7,))
    assert len(hwc.detect()) > 0
