"""Frame metering on the GPU (irmv_engine_meter / irmv_engine_set_metering, csrc/k_meter.hip): every record equals, bit for
bit, the host reference irmv_detection_amd/metering.py applied to the frame the engine itself hands out -- get_rotated_image()
turned back into the frame as stored, or the raw slot -- and every case also asserts hist.sum(1) == n == the n[4] of
irmv_meter_map.  One-slot engines at a 64 x 64 net unless stated.  tests/test_metering.py checks the reference itself.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import detect_craft as dc
from irmv_detection_amd import bayer, capi, metering, window
from irmv_detection_amd.engine import YoloEngine
from test_metering import tinted_scene

pytestmark = pytest.mark.gpu

PATTERN_OF = {v: k for k, v in capi.BAYER_FORMATS.items()}
STEPS = (1, 2, 4)
# whole view, inside at an odd corner, clipped on both sides, empty (wholly outside)
RECTS = (None, (13, 7, 51, 33), (-5, 40, 30, 60), (88, -3, 40, 20), (100, 0, 5, 5), (-9, -9, 9, 9))
PARITY_RECTS = ((12, 6, 40, 30), (13, 6, 40, 30), (12, 7, 40, 30), (13, 7, 41, 31))


@pytest.fixture(scope="module")
def cblob(blob):
    """Every anchor a candidate of two classes, an armor-like quad around it: detections on every frame."""
    return dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))


def frame_of(w, h, seed, channels=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, channels) if channels else (h, w), dtype=np.uint8)


def eng(blob, size, **kw):
    return YoloEngine(None, size, weights_blob=blob, net_size=64, **kw)


def view_of(e, slot):
    return e.view(slot) if e.window_size else ("window", e.src_image_size)


def reference(e, domain, rect, step, slot=0):
    """metering.py on the frame the engine hands out."""
    rot = e._rotate180
    name, size = view_of(e, slot)
    if domain == "view":
        stored = np.ascontiguousarray(e.get_rotated_image(slot)[::-1, ::-1])
        assert stored.shape[:2] == (size[1], size[0])
        return metering.meter(stored, rect, step, "view", rot)
    corner = (0, 0)
    if e.window_size and name == "window":
        x0, y0, w, h = e.window(slot)
        corner = window.buffer_origin(e.src_image_size, x0, y0, w, h, rot)
    return metering.meter(e.get_src_image_buffer(slot), rect, step, "raw", rot, PATTERN_OF[e.src_format], size, corner)


def map_n(e, domain, rect, step, slot=0):
    view = capi.VIEWS[view_of(e, slot)[0]]
    win_xy = e.window(slot)[:2] if e.window_size else (0, 0)
    return capi.meter_map(e.src_image_size, capi.meter_opts(domain, rect, step), view, e.window_size, win_xy, e._rotate180, e.src_format, net_size=64)["n"]


def same(got, exp, n, what):
    assert np.array_equal(got["hist"], exp["hist"]), what
    assert np.array_equal(got["n"], exp["n"]) and tuple(got["rect"]) == tuple(exp["rect"]), what
    assert (got["domain"], got["step"]) == (exp["domain"], exp["step"]), what
    assert tuple(int(v) for v in got["hist"].sum(1)) == tuple(int(v) for v in got["n"]) == tuple(n), what


def check(e, domain, rect, step, slot=0):
    exp = reference(e, domain, rect, step, slot)
    same(e.meter(domain, rect, step, slot), exp, map_n(e, domain, rect, step, slot), (domain, rect, step, slot))
    return exp


def sweep(e, domain="view", rects=RECTS, slot=0):
    total = 0
    for rect, step in itertools.product(rects, STEPS):
        total += int(check(e, domain, rect, step, slot)["n"][3])
    assert total > 0


# ---- on demand -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", (True, False))
def test_hwc(cblob, rot):
    with eng(cblob, (100, 68), rotate180=rot) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 1)
        sweep(e)
        assert e.meter("view", (100, 0, 5, 5))["hist"].sum() == 0


def test_odd_rows_of_303_bytes(cblob):
    with eng(cblob, (101, 67)) as e:
        e.get_src_image_buffer()[:] = frame_of(101, 67, 2)
        sweep(e, rects=(None, (13, 7, 51, 33), (0, 0, 101, 1), (100, 0, 1, 67), (1, 1, 99, 65), (50, 66, 60, 9)))


def test_uniform_frames(cblob):
    with eng(cblob, (100, 68)) as e:
        for v in (0, 255):
            e.get_src_image_buffer()[:] = v
            for step in STEPS:
                exp = check(e, "view", None, step)
                assert exp["hist"][:, v].tolist() == exp["n"].tolist()


@pytest.mark.parametrize("merge", ("1", "0"))
def test_flat_runs_between_noise_in_both_forms_of_the_add(cblob, monkeypatch, merge):
    """Lane-groups of equal pixels (added once with their count) beside groups that are not, in the kernel's two instantiations
    (IRMV_METER_MERGE): the same bits."""
    monkeypatch.setenv("IRMV_METER_MERGE", merge)
    f = frame_of(100, 68, 12)
    f[:, 20:75] = (7, 200, 31)                                    # flat runs that start and end inside lane-groups
    f[30:40] = 255
    raw = frame_of(100, 68, 13, channels=0)
    raw[:, 10:81] = 90
    raw[1::2, 24:60] = 17                                         # cell rows (90, 90) and (17, 17): G and B differ from R
    with eng(cblob, (100, 68)) as e:
        e.get_src_image_buffer()[:] = f
        sweep(e, rects=(None, (13, 7, 51, 33), (21, 0, 50, 68)))
    with eng(cblob, (100, 68), src_format="GBRG", rotate180=False) as e:
        e.get_src_image_buffer()[:] = raw
        sweep(e, "raw", (None, (13, 7, 51, 33), (11, 1, 64, 60)))


def test_three_slots_of_a_size_that_is_6_mod_16(cblob):
    with eng(cblob, (322, 201), num_slots=3) as e:
        assert (322 * 201 * 3) % 16 == 6
        for s in range(2):
            e.get_src_image_buffer(s)[:] = frame_of(322, 201, 3 + s)
        last = e.get_src_image_buffer(2)
        last[:] = 0
        last[200, 321, 2] = 255                                   # slot 2's only non-zero byte is its last
        for s in range(3):
            for rect, step in ((None, 1), (None, 2), ((1, 1, 320, 199), 1), ((0, 0, 3, 3), 4), ((5, 3, 311, 190), 4)):
                check(e, "view", rect, step, s)
        assert e.meter("view", None, 1, 2)["hist"][2, 255] == 1


def test_three_partial_workgroups(cblob):
    L = capi.meter_limits()
    rows = 2 * L["rows_per_block"] + 5                             # at least three partial workgroups per frame
    assert -(-rows // L["rows_per_block"]) >= 3 <= L["blocks_max"]
    with eng(cblob, (52, rows)) as e:
        e.get_src_image_buffer()[:] = frame_of(52, rows, 5)
        sweep(e, rects=(None, (3, 1, 45, rows - 2), (0, rows - 1, 52, 1)))


@pytest.mark.parametrize("rot", (True, False))
@pytest.mark.parametrize("pattern", bayer.PATTERNS)
def test_bayer_raw(cblob, pattern, rot):
    with eng(cblob, (100, 68), src_format=pattern, rotate180=rot) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 6, channels=0)
        sweep(e, "raw", (None,) + PARITY_RECTS + ((99, 0, 5, 68), (97, 66, 9, 9)))
        n = e.meter("raw", None, 1)["n"]
        assert n.tolist() == [1700, 3400, 1700, 6800]
        assert e.meter("raw", (99, 0, 5, 68))["hist"].sum() == 0     # one column: no whole cell


@pytest.mark.parametrize("algo", ("bilinear", "mhc"))
def test_bayer_view_behind_gains_and_lut(cblob, algo):
    lut = np.stack([np.clip(np.arange(256) * 1.3, 0, 255), 255 - np.arange(256), (np.arange(256) // 3) * 3]).astype(np.uint8)
    with eng(cblob, (100, 68), src_format="GRBG", bayer_demosaic=algo) as e:
        raw = frame_of(100, 68, 7, channels=0)
        e.get_src_image_buffer()[:] = raw
        e.set_bayer_isp((300, 256, 200), lut)
        stored = bayer.demosaic(raw, "GRBG", (300, 256, 200), algo, lut)
        assert np.array_equal(e.get_rotated_image()[::-1, ::-1], stored)
        sweep(e, "view", (None, (13, 7, 51, 33)))
        before = check(e, "raw", None, 1)                           # RAW sees through gains and LUT
        e.set_bayer_isp((256, 256, 256))
        same(e.meter("raw"), before, map_n(e, "raw", None, 1), "raw after a new isp")


@pytest.mark.parametrize("src_format", (capi.SRC_HWC8, "BGGR"))
def test_window_engine_in_both_views(cblob, src_format):
    hwc = src_format == capi.SRC_HWC8
    domains = ("view",) if hwc else ("view", "raw")
    with eng(cblob, (160, 128), window=(100, 68), src_format=src_format) as e:
        e.get_src_image_buffer()[:] = frame_of(160, 128, 8, channels=3 if hwc else 0)
        for corner in ((13, 7), (60, 60)):                         # an odd corner; the bottom-right corner
            e.set_window(*corner)
            for d in domains:
                sweep(e, d, (None, (13, 7, 51, 33), (-5, 40, 30, 60)))
        e.set_view("frame")
        for d in domains:
            sweep(e, d, (None, (13, 7, 51, 33), (100, 90, 90, 90)))
        e.set_view("window")
        check(e, domains[-1], None, 1)
    if hwc:
        with eng(cblob, (160, 128), window=(100, 68)) as e:
            with pytest.raises(capi.IrmvError) as ei:
                e.meter("raw")
            assert ei.value.code == capi.ERR_ARG


# ---- in the step -----------------------------------------------------------------------------------------------------------
def graph_ops(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_ops(e._h, None, 0, C.byref(n)))
    arr = (capi.GraphOp * n.value)()
    capi.check(e._L.irmv_engine_ops(e._h, arr, n.value, C.byref(n)))
    return [o.kind.decode() for o in arr]


def hip_memcpy_h2d(dst_ptr, arr):
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(arr)
    assert hip.hipMemcpy(C.c_void_p(dst_ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0


def step_equals_meter(e, domain, rect, step, slot=0):
    """frame_stats of the slot's step == meter() == the reference."""
    got = e.frame_stats(slot)
    exp = reference(e, domain, rect, step, slot)
    n = map_n(e, domain, rect, step, slot)
    same(got, exp, n, ("step", domain, rect, step, slot))
    same(e.meter(domain, rect, step, slot), exp, n, ("meter", domain, rect, step, slot))
    same(e.frame_stats(slot), exp, n, "the on-demand call leaves the step's record alone")


@pytest.mark.parametrize("form", ("graph", "eager"))
@pytest.mark.parametrize("window_upload", ("1", "0"))
def test_step_record_in_every_launch_and_upload_form(cblob, monkeypatch, form, window_upload):
    monkeypatch.setenv("IRMV_SYNC_LAUNCH", form)
    monkeypatch.setenv("IRMV_WINDOW_UPLOAD", window_upload)
    with eng(cblob, (160, 128), window=(100, 68)) as e:           # the crop out of the pinned slot, or upload + crop
        assert e.sync_launch == form
        e.get_src_image_buffer()[:] = frame_of(160, 128, 9)
        e.set_window(13, 7)
        assert "meter" not in graph_ops(e)
        e.set_metering("view", (13, 7, 51, 33), 2)
        assert graph_ops(e).count("meter") == 1
        assert len(e.detect()) > 0
        step_equals_meter(e, "view", (13, 7, 51, 33), 2)
        e.set_view("frame")
        assert len(e.detect()) > 0
        step_equals_meter(e, "view", (13, 7, 51, 33), 2)
        assert graph_ops(e).count("meter") == 1
    with eng(cblob, (100, 68), src_format="RGGB") as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 10, channels=0)
        e.set_metering("raw", (13, 7, 41, 31), 1)
        e.detect()
        step_equals_meter(e, "raw", (13, 7, 41, 31), 1)


def test_batched_async_and_device_resident_steps(cblob):
    fr = [frame_of(100, 68, 20 + s) for s in range(3)]
    with eng(cblob, (100, 68), num_slots=3) as e:
        e.set_metering("view", None, 1)
        for s in range(3):
            e.get_src_image_buffer(s)[:] = fr[s]
        e.submit(0, 3)                                            # one batched step, three different frames
        e.wait()
        for s in range(3):
            assert len(e.results(s)) > 0
            step_equals_meter(e, "view", None, 1, s)
        assert not np.array_equal(e.frame_stats(0)["hist"], e.frame_stats(1)["hist"])
        e.set_metering("view", (13, 7, 51, 33), 4)
        for s in range(3):
            e.get_src_image_buffer(s)[:] = fr[(s + 1) % 3]
        for s in range(3):                                        # three single-slot submits in flight
            e.submit(s, 1, async_upload=True)
        for s in range(3):
            e.wait_slots(s, 1)
            exp = metering.meter(fr[(s + 1) % 3], (13, 7, 51, 33), 4, "view", True)
            same(e.frame_stats(s), exp, map_n(e, "view", (13, 7, 51, 33), 4, s), ("async", s))
        e.wait()
        for s in range(3):                                        # device-resident frames: nothing is uploaded
            hip_memcpy_h2d(e.src_device_ptr(s), fr[(s + 2) % 3])
        e.submit(0, 3, h2d=False)
        e.wait()
        for s in range(3):
            exp = metering.meter(fr[(s + 2) % 3], (13, 7, 51, 33), 4, "view", True)
            same(e.frame_stats(s), exp, map_n(e, "view", (13, 7, 51, 33), 4, s), ("device", s))


def test_a_batch_over_the_block_cap(cblob):
    """A launch of more than batch_frames frames takes at most blocks_batch partial workgroups per frame: a frame with more
    rows than those cover at rows_per_block each, once alone (blocks_max) and once in such a batch."""
    L = capi.meter_limits()
    rows, n = L["rows_per_block"] * L["blocks_batch"] + 9, L["batch_frames"] + 1
    assert -(-rows // L["rows_per_block"]) > L["blocks_batch"] and L["blocks_max"] > L["blocks_batch"]
    fr = [frame_of(36, rows, 40 + s) for s in range(n)]
    with eng(cblob, (36, rows), num_slots=n, num_streams=1) as e:   # (one stream: the submit is ONE launch of n frames)
        e.set_metering("view", (1, 1, 33, rows - 2), 1)
        for s in range(n):
            e.get_src_image_buffer(s)[:] = fr[s]
        e.submit(0, n)
        e.wait()
        for s in range(n):
            step_equals_meter(e, "view", (1, 1, 33, rows - 2), 1, s)
        e.detect(n - 1)
        step_equals_meter(e, "view", (1, 1, 33, rows - 2), 1, n - 1)


def test_records_are_those_of_an_engine_that_never_metered(cblob):
    f = frame_of(100, 68, 30)
    with eng(cblob, (100, 68)) as plain, eng(cblob, (100, 68)) as e:
        plain.get_src_image_buffer()[:] = f
        e.get_src_image_buffer()[:] = f
        plain.detect()
        want = [bytes(d) for d in plain.results_raw()]
        assert len(want) > 0
        ops = graph_ops(plain)
        assert "meter" not in ops and graph_ops(e) == ops
        with pytest.raises(capi.IrmvError) as ei:
            e.frame_stats()                                       # before any enable
        assert ei.value.code == capi.ERR_ARG
        e.set_metering(None)                                      # off on an engine that was never on: nothing happens
        assert graph_ops(e) == ops
        with pytest.raises(capi.IrmvError):
            e.frame_stats()
        same(e.meter("view"), reference(e, "view", None, 1), map_n(e, "view", None, 1), "on demand, never enabled")
        assert graph_ops(e) == ops                                # the on-demand call enables nothing
        e.detect()
        assert [bytes(d) for d in e.results_raw()] == want
        e.set_metering("view")
        assert graph_ops(e) == ops + ["meter"]
        e.detect()
        assert [bytes(d) for d in e.results_raw()] == want
        step_equals_meter(e, "view", None, 1)
        assert graph_ops(plain) == ops


def test_new_options_and_off_recapture_nothing(cblob):
    with eng(cblob, (100, 68)) as e:
        e.get_src_image_buffer()[:] = frame_of(100, 68, 31)
        e.detect()
        e.set_metering("view", None, 1)
        e.detect()
        graphs = e.debug_graph_count()
        step_equals_meter(e, "view", None, 1)
        e.set_metering("view", (13, 7, 51, 33), 2)                # a changed rectangle and step
        e.detect()
        step_equals_meter(e, "view", (13, 7, 51, 33), 2)
        e.set_metering(None)                                      # off: the record is all zero
        e.detect()
        off = e.frame_stats()
        assert off["hist"].sum() == 0 and off["n"].sum() == 0 and off["rect"] == (0, 0, 0, 0) and (off["domain"], off["step"]) == (0, 0)
        on, o = C.c_int(1), capi.meter_opts()
        capi.check(e._L.irmv_engine_get_metering(e._h, C.byref(o), C.byref(on)))
        assert on.value == 0
        e.set_metering("view", (-5, 40, 30, 60), 4)               # on again
        e.detect()
        step_equals_meter(e, "view", (-5, 40, 30, 60), 4)
        capi.check(e._L.irmv_engine_get_metering(e._h, C.byref(o), C.byref(on)))
        assert on.value == 1 and (o.x0, o.y0, o.w, o.h, o.step, o.domain) == (-5, 40, 30, 60, 4, 0)
        assert e.debug_graph_count() == graphs
        with pytest.raises(capi.IrmvError):
            e.set_metering("raw")                                 # refused on an HWC engine, and nothing changes
        bad = capi.meter_opts("view", None, 3)
        assert e._L.irmv_engine_set_metering(e._h, C.byref(bad)) == capi.ERR_ARG
        assert e._L.irmv_engine_meter(e._h, 0, C.byref(bad), C.byref(capi.FrameStats())) == capi.ERR_ARG
        assert e._L.irmv_engine_meter(e._h, 1, C.byref(o), C.byref(capi.FrameStats())) == capi.ERR_ARG
        e.detect()
        step_equals_meter(e, "view", (-5, 40, 30, 60), 4)
        assert e.debug_graph_count() == graphs


@pytest.mark.parametrize("pattern", ("RGGB", "GBRG"))
def test_white_balance_closes_on_the_engine(cblob, pattern):
    raw = tinted_scene(pattern)
    with eng(cblob, (100, 68), src_format=pattern) as e:
        e.get_src_image_buffer()[:] = raw
        e.set_metering("raw")
        e.detect()
        rec = e.frame_stats()
        same(rec, metering.meter(raw, None, 1, "raw", True, pattern), map_n(e, "raw", None, 1), "raw record")
        gains = capi.stats_gray_world(rec, 8, 247)
        assert gains == metering.gray_world(rec, 8, 247)
        e.set_bayer_isp(gains)
        e.set_metering("view")
        e.detect()
        exp = metering.meter(bayer.demosaic(raw, pattern, gains), None, 1, "view", True)
        same(e.frame_stats(), exp, map_n(e, "view", None, 1), "view record behind the new gains")
        means = [metering.mean_q8(exp, c)[0] / 256.0 for c in range(3)]
        assert max(means) - min(means) < 1.0
