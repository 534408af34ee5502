"""Tracking window on the GPU: a window engine at (x0, y0) on a frame is, bit for bit, a PLAIN engine whose source size
is the window, whose camera has the principal point moved by (x0, y0), fed irmv_detection_amd.window.crop of the frame --
boxes and keypoints shifted by the corner in fp32.  The plain engine is the reference throughout (P below); the host
crop is numpy slicing.

The full frame is 322 x 201 HWC: a row pitch of 966 bytes and a frame of 194,166 bytes (= 6 mod 16), so no row and no
slot end is 16-byte aligned; the window is 256 x 128 into a 128 x 64 net (exactly 2 : 1) unless a test says otherwise.

The session blob's class logits stay below the score threshold at these sizes, so the tests run on a blob whose class
biases are shifted up (the logits still come from the frame through every layer) and whose keypoint branch gives an
armor-like quad around each anchor (tests/detect_craft.py): every compared frame holds detections with a solved pose, which
each test asserts.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import rect_ref
from conftest import K_REF
from irmv_detection_amd import bayer, capi, frames, window
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle

pytestmark = pytest.mark.gpu

FULL, WIN, NET = (322, 201), (256, 128), (128, 64)
K = tuple(float(v) for v in K_REF)


@pytest.fixture(scope="module")
def wblob(blob):
    return dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))


def weng(blob, full=FULL, win=WIN, net=NET, **kw):
    kw.setdefault("camera_matrix", K)
    return YoloEngine(None, full, weights_blob=blob, net_size=net[0], net_height=net[1], window=win, **kw)


def peng(blob, win=WIN, net=NET, org=(0, 0), **kw):
    """The reference: a plain engine on the window-sized source, principal point moved by the corner (Python doubles)."""
    kw.pop("camera_matrix", None)
    return YoloEngine(None, win, weights_blob=blob, net_size=net[0], net_height=net[1],
                      camera_matrix=window.shifted_camera(K, org[0], org[1]), **kw)


def dets_of(e, slot):
    """The slot's irmv_det records as plain tuples of arrays."""
    n = C.c_int(0)
    buf = (capi.Det * e.max_det)()
    capi.check(e._L.irmv_engine_results(e._h, slot, buf, e.max_det, C.byref(n)))
    out = []
    for i in range(n.value):
        d = buf[i]
        out.append(dict(xyxy=np.array(d.xyxy, np.float32), kpts=np.array(d.kpts, np.float32), score=np.float32(d.score),
                        ints=(d.class_id, d.anchor, d.pnp_ok, d.armor_valid, d.armor_size, d.n_lights),
                        pose=np.concatenate([np.array(d.rvec), np.array(d.tvec), np.array(d.quat)])))
    return out


RAW_KEYS = ("boxes", "scores", "classes", "anchors", "kpts")


def snapshot(e, slot, tensors=True):
    raw = e.read_raw(slot)
    s = dict(dets=dets_of(e, slot), raw={k: raw[k].copy() for k in RAW_KEYS}, counts=(raw["num_dets"], raw["n_candidates"]))
    if tensors:
        s["input"], s["head"] = e.read_input(slot), e.read_head(slot)
    return s


_refs = {}


def reference(blob, frame, org, rot=True, win=WIN, net=NET, tag="", **kw):
    """P's snapshot on the crop at `org`, computed once per case and shared."""
    key = (tag, org, rot, win, net, tuple(sorted(kw.items())))
    if key not in _refs:
        with peng(blob, win, net, org, rotate180=rot, **kw) as p:
            p.get_src_image_buffer()[:] = window.crop(frame, org[0], org[1], win[0], win[1], rot)
            p.detect()
            _refs[key] = snapshot(p, 0)
    return _refs[key]


def same_tensors(got, ref):
    assert np.array_equal(got["input"], ref["input"])
    assert np.array_equal(got["head"], ref["head"])


def same_results(got, ref, org, where=""):
    """raw (net-input pixels) equal; every irmv_det field equal, xyxy and kpts = float32(P) + float32(corner).
    Returns the number of detections with a solved pose."""
    assert got["counts"] == ref["counts"], (where, got["counts"], ref["counts"])
    for k in RAW_KEYS:
        assert np.array_equal(got["raw"][k], ref["raw"][k]), (where, k)
    assert len(got["dets"]) == len(ref["dets"]), where
    o4 = np.array([org[0], org[1], org[0], org[1]], np.float32)
    o8 = np.tile(np.array(org, np.float32), 4)
    for i, (g, r) in enumerate(zip(got["dets"], ref["dets"])):
        assert g["ints"] == r["ints"] and g["score"] == r["score"], (where, i)
        assert g["pose"].tobytes() == r["pose"].tobytes(), (where, i)
        assert np.array_equal(g["xyxy"], r["xyxy"] + o4), (where, i)
        assert np.array_equal(g["kpts"], r["kpts"] + o8), (where, i)
    return sum(d["ints"][2] == 1 for d in got["dets"])


def frame_of(i, size=FULL):
    return frames.synthetic_frame(i, size[0], size[1])


# ---- 1. every source alignment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False])
def test_every_source_alignment(wblob, rot):
    """x0 = 0 .. 15: all sixteen values of 3 x0 mod 16 at the start of a source row; y0 walks the top, the middle and the
    bottom of the frame.  One window engine against one P: tensors and net-pixel results do not depend on the camera."""
    frame = frame_of(11)
    assert (FULL[0] * 3) % 16 != 0 and (FULL[0] * FULL[1] * 3) % 16 == 6
    solved = 0
    with weng(wblob, rotate180=rot) as w, peng(wblob, rotate180=rot) as p:
        assert w.window() == ((FULL[0] - WIN[0]) // 2, (FULL[1] - WIN[1]) // 2, WIN[0], WIN[1])   # centred at creation
        assert w.get_src_image_buffer().shape == (FULL[1], FULL[0], 3) and w._L.irmv_engine_src_bytes(w._h) == FULL[0] * FULL[1] * 3
        w.get_src_image_buffer()[:] = frame
        seen = set()
        for x0 in range(16):
            y0 = (0, 37, 73)[x0 % 3]
            w.set_window(x0, y0)
            assert w.window()[:2] == (x0, y0)
            w.detect()
            crop = window.crop(frame, x0, y0, WIN[0], WIN[1], rot)
            p.get_src_image_buffer()[:] = crop
            p.detect()
            got, ref = snapshot(w, 0), snapshot(p, 0)
            same_tensors(got, ref)
            assert np.array_equal(got["input"], rect_ref.preprocess(crop, NET[0], NET[1], capi.RESIZE_STRETCH, rot))
            assert got["counts"] == ref["counts"] and all(np.array_equal(got["raw"][k], ref["raw"][k]) for k in RAW_KEYS), (x0, y0)
            solved += sum(d["ints"][2] == 1 for d in got["dets"])
            seen.add((3 * window.buffer_origin(FULL, x0, y0, WIN[0], WIN[1], rot)[0]) % 16)
        assert seen == set(range(16))
    assert solved > 0


# ---- 2. full equivalence including pose ------------------------------------------------------------------------------------
def test_full_equivalence_including_pose(wblob):
    frame = frame_of(12)
    with weng(wblob) as w:
        w.get_src_image_buffer()[:] = frame
        for org in [(0, 0), (66, 73), (31, 40)]:       # both extreme corners of the buffer, and an interior window
            w.set_window(*org)
            w.detect()
            got, ref = snapshot(w, 0), reference(wblob, frame, org, tag="f12")
            same_tensors(got, ref)
            assert same_results(got, ref, org, org) > 0


@pytest.mark.parametrize("rot", [True, False])
def test_last_slot_at_the_last_byte(wblob, rot):
    """Slot 2 of 3 with the window in the buffer's bottom-right corner: its last row ends at the last byte of the device
    frames and of the pinned slots."""
    frame = frame_of(13)
    org = (0, 0) if rot else (66, 73)
    assert window.buffer_origin(FULL, org[0], org[1], WIN[0], WIN[1], rot) == (66, 73)
    with weng(wblob, num_slots=3, rotate180=rot) as w:
        w.get_src_image_buffer(2)[:] = frame
        w.set_window(org[0], org[1], slot=2)
        w.detect(2)                                     # the crop reads the pinned slot
        ref = reference(wblob, frame, org, rot, tag="f13")
        got = snapshot(w, 2)
        same_tensors(got, ref)
        assert same_results(got, ref, org, "pinned") > 0
        w.submit(2, 1, async_upload=True)               # the band upload ends at the device frames' last byte
        w.wait()
        assert same_results(snapshot(w, 2, False), ref, org, "band") > 0
        w.submit(0, 3)                                  # ... and the batched crop reads it there
        w.wait()
        assert same_results(snapshot(w, 2, False), ref, org, "batched") > 0


def test_window_at_one_to_one(wblob):
    frame = frame_of(14)
    win = (128, 64)
    with weng(wblob, win=win) as w:
        w.get_src_image_buffer()[:] = frame
        for org in [(97, 68), (194, 137), (0, 0)]:
            w.set_window(*org)
            w.detect()
            crop = window.crop(frame, org[0], org[1], win[0], win[1])
            got, ref = snapshot(w, 0), reference(wblob, frame, org, win=win, tag="f14")
            same_tensors(got, ref)
            assert np.array_equal(got["input"], rect_ref.preprocess(crop, NET[0], NET[1]))
            assert same_results(got, ref, org, org) > 0
            assert np.array_equal(w.get_rotated_image(), crop[::-1, ::-1])


def test_window_equal_to_the_full_frame_is_the_plain_engine(wblob):
    full = (320, 200)
    frame = frame_of(15, full)
    with weng(wblob, full=full, win=full) as w, YoloEngine(None, full, weights_blob=wblob, net_size=NET[0], net_height=NET[1], camera_matrix=K) as p:
        assert w.window() == (0, 0, 320, 200)
        for e in (w, p):
            e.get_src_image_buffer()[:] = frame
            e.detect()
        got, ref = snapshot(w, 0), snapshot(p, 0)
        same_tensors(got, ref)
        assert same_results(got, ref, (0, 0)) > 0
        with pytest.raises(capi.IrmvError):
            w.set_window(1, 0)


# ---- 3. every launch form ----------------------------------------------------------------------------------------------------
def _hip_memcpy_h2d(dst_ptr, arr):
    """hipMemcpy through the HIP runtime libirmv_hip.so already loaded (same SONAME: dlopen returns that library)."""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(arr)
    assert hip.hipMemcpy(C.c_void_p(dst_ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice


ORIGINS8 = [(0, 0), (66, 73), (5, 37), (66, 0), (0, 73), (31, 40), (13, 9), (50, 70)]


def test_every_launch_form_gives_the_same_bits(wblob, monkeypatch):
    fr = [frame_of(40 + i) for i in range(8)]
    refs = [reference(wblob, fr[s], ORIGINS8[s], tag=f"f{40 + s}") for s in range(8)]     # frame s always travels with origin s
    solved, forms = 0, set()

    def place(w, perm):
        """frame / origin s into slot perm[s]"""
        for s in range(8):
            w.get_src_image_buffer(perm[s])[:] = fr[s]
            w.set_window(*ORIGINS8[s], slot=perm[s])

    def check(w, perm, what, tensors=False):
        n = 0
        for s in range(8):
            got = snapshot(w, perm[s], tensors and s < 2)
            if tensors and s < 2:
                same_tensors(got, refs[s])
            n += same_results(got, refs[s], ORIGINS8[s], (what, s))
        assert n > 0, what
        forms.add(what)
        return n

    ident = list(range(8))
    for mode in ("graph", "eager"):
        for wu in ("1", "0"):
            monkeypatch.setenv("IRMV_SYNC_LAUNCH", mode)
            monkeypatch.setenv("IRMV_WINDOW_UPLOAD", wu)
            with weng(wblob, num_slots=8, num_streams=2) as w:
                assert w.sync_launch == mode
                place(w, ident)
                for s in range(8):
                    w.detect(s)
                solved += check(w, ident, f"detect {mode} upload={wu}", tensors=True)
                if (mode, wu) != ("graph", "1"):
                    continue
                # batched submit(H2D): 8 slots on 2 streams, whole-frame uploads inside the graphs
                perm = [(s + 3) % 8 for s in range(8)]
                place(w, perm)
                w.submit(0, 8)
                w.wait()
                check(w, perm, "batched")
                # eight single-slot ASYNC_UPLOAD submits in flight: band copies on the upload stream
                perm = [7 - s for s in range(8)]
                place(w, perm)
                for s in range(8):
                    w.submit(s, 1, async_upload=True)
                for s in range(8):
                    w.wait_slots(s, 1)
                check(w, perm, "async bands")
                w.wait()
                # a device-resident producer: full frames written into the device slots, submitted without H2D
                place(w, ident)
                for s in range(8):
                    w.get_src_image_buffer(s)[:] = 0
                    _hip_memcpy_h2d(w.src_device_ptr(s), fr[s])
                w.submit(0, 8, h2d=False)
                w.wait()
                check(w, ident, "device, eight at once")
                w.submit(2, 1, h2d=False)
                w.wait()
                assert same_results(snapshot(w, 2, False), refs[2], ORIGINS8[2], "device, one alone") > 0
                forms.add("device, one alone")
    assert len(forms) == 8 and solved > 0


# ---- 4. moving the window ----------------------------------------------------------------------------------------------------
def test_moving_the_window(wblob):
    frame = frame_of(16)
    a, b = (3, 70), (60, 2)
    ra, rb = reference(wblob, frame, a, tag="f16"), reference(wblob, frame, b, tag="f16")
    with weng(wblob, num_slots=2) as w:
        for s in range(2):
            w.get_src_image_buffer(s)[:] = frame
        w.set_window(*a, slot=1)
        w.detect(1)
        assert same_results(snapshot(w, 1, False), ra, a, "first") > 0
        w.set_window(*b, slot=1)
        # results read after a later set_window still carry the corner their step was submitted with
        assert same_results(snapshot(w, 1, False), ra, a, "after the move") > 0
        w.detect(1)
        got = snapshot(w, 1)
        same_tensors(got, rb)
        assert same_results(got, rb, b, "second") > 0
        # a set_window between two asynchronous submits of one slot leaves the first with the old window
        w.set_window(*a, slot=0)
        w.submit(0, 1, async_upload=True)
        w.set_window(*b, slot=0)                        # waits for the step in flight, then moves
        assert w.window(0)[:2] == b
        assert same_results(snapshot(w, 0, False), ra, a, "in flight") > 0
        w.submit(0, 1, async_upload=True)
        w.wait_slots(0, 1)
        assert same_results(snapshot(w, 0, False), rb, b, "moved") > 0
        # set_window_center clamps into the frame
        assert w.set_window_center(0.0, 500.0, slot=0) == (0, 73) and w.window(0) == (0, 73, 256, 128)
        assert w.set_window_center(161.0, 100.0, slot=0) == (33, 36)
        assert w.set_window_center(1e4, -5.0, slot=0) == (66, 0)


def test_profile_lists_the_crop_once_per_step_of_a_window_engine_only(wblob, monkeypatch):
    # what is compared is the step's SHAPE: both engines take the untimed choices (the tiles as configured, no timed grouping
    # of the Detect branches -- at this net size two group tiles time alike and two engines may pick differently)
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_HEAD", "0")
    with peng(wblob, num_slots=2) as p:
        plain = {c: [k["name"] for k in p.profile(0, c)] for c in (1, 2)}
    assert not any("window_crop" in n for names in plain.values() for n in names)
    with weng(wblob, num_slots=2) as w:
        kinds = [(o.kind.decode(), o.kname.decode()) for o in _ops(w)]
        assert kinds[0] == ("crop", "window_crop") and sum(k == "crop" for k, _ in kinds) == 1
        for c in (1, 2):
            prof = w.profile(0, c)
            assert [k["name"] for k in prof] == ["window_crop"] + plain[c]      # one op in front of the unchanged step
            assert prof[0]["bytes"] == 2 * WIN[0] * WIN[1] * 3 * c and prof[0]["ms"] > 0
    with weng(wblob, full=(322, 202), src_format="GRBG", num_slots=2) as w:
        names = [k["name"] for k in w.profile(0, 1)]
        assert names[:2] == ["bayer_demosaic", "window_crop"] and names[2:] == plain[1]


def _ops(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_ops(e._h, None, 0, C.byref(n)))
    ops = (capi.GraphOp * n.value)()
    capi.check(e._L.irmv_engine_ops(e._h, ops, n.value, C.byref(n)))
    return list(ops)


# ---- 5. Bayer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bilinear", "mhc"])
def test_bayer_window_engine_is_the_hwc_window_engine_on_the_demosaiced_frame(wblob, algo):
    """The demosaic runs on the whole raw frame, the crop behind it: any window, any origin, odd ones included."""
    full, pattern = (322, 202), "GRBG"
    raw = bayer.mosaic(frame_of(17, full), pattern)
    gains, lut = (300, 256, 420), (255 - np.arange(256)).astype(np.uint8)
    solved = 0
    with weng(wblob, full=full, src_format=pattern, bayer_demosaic=algo, num_slots=2) as be, weng(wblob, full=full, num_slots=2) as he:
        assert be.get_src_image_buffer().shape == (202, 322) and be._L.irmv_engine_src_bytes(be._h) == 322 * 202
        for isp in (None, (gains, lut)):
            hwc = bayer.demosaic(raw, pattern, algo=algo) if isp is None else bayer.demosaic(raw, pattern, gains, algo, lut)
            if isp is not None:
                be.set_bayer_isp(gains, lut)
            for s in range(2):
                be.get_src_image_buffer(s)[:] = raw
                he.get_src_image_buffer(s)[:] = hwc
            for org in [(0, 0), (66, 74), (31, 41)]:
                for e in (be, he):
                    e.set_window(*org)
                    e.detect()
                got, ref = snapshot(be, 0), snapshot(he, 0)
                same_tensors(got, ref)
                solved += same_results(got, ref, (0, 0), (algo, isp is not None, org))   # both already carry the corner
                assert np.array_equal(be.get_rotated_image(), window.crop(hwc, org[0], org[1], WIN[0], WIN[1])[::-1, ::-1])
            for e in (be, he):                          # batched: one demosaic and one crop launch for both frames
                e.set_window(9, 70, slot=1)
                e.submit(0, 2)
                e.wait()
            for s in range(2):
                solved += same_results(snapshot(be, s, False), snapshot(he, s, False), (0, 0), (algo, "batched", s))
    assert solved > 0


# ---- 6. classical point source ----------------------------------------------------------------------------------------------
def test_classical_points_in_a_window_over_the_armor(blob, rm_test_image):
    """rm_test.jpg, a 640 x 512 window over the armor at the sensor's resolution.  The blob's Detect finals are crafted so
    that the step's boxes are known: level 2 only, 192 x 192 boxes on a grid one of which holds the armor's two lights."""
    full, win, net, org, rot = (1280, 1024), (640, 512), (640, 512), (400, 150), False
    lit = {0: ("bias", dc.dark_bias(14)), 1: ("bias", dc.dark_bias(14)), 2: ("bias", dc.two_tied_bias(14))}
    b = dc.craft(blob, cls=lit, box=("bias", dc.dfl_bias(3)))
    kw = dict(point_source=capi.POINTS_CLASSICAL, rotate180=rot, armor_size=capi.ARMOR_LARGE)
    crop = window.crop(rm_test_image, org[0], org[1], win[0], win[1], rot)
    with weng(b, full, win, net, **kw) as w, peng(b, win, net, org, **kw) as p:
        w.get_src_image_buffer()[:] = rm_test_image
        w.set_window(*org)
        p.get_src_image_buffer()[:] = crop
        w.detect()
        p.detect()
        got, ref = snapshot(w, 0, False), snapshot(p, 0, False)
        assert same_results(got, ref, org, "in step") > 0
        assert any(d["ints"][3] == 1 and d["ints"][5] == 2 for d in got["dets"])
        # extract_armors: boxes in full coordinates against P on the shifted boxes
        boxes = np.array([[630, 360, 785, 420], [600, 340, 820, 440], [500, 300, 900, 500], [630, 360, 700, 420], [420, 160, 1030, 650],
                          [100, 100, 300, 300]], np.float32)
        o4 = np.array([org[0], org[1], org[0], org[1]], np.float32)
        ga, ra = w.extract_armors_raw(boxes), p.extract_armors_raw(boxes - o4)
        n = 0
        for i in range(len(boxes)):
            g, r = ga[i], ra[i]
            assert (g.pnp_ok, g.armor_valid, g.armor_size, g.n_lights) == (r.pnp_ok, r.armor_valid, r.armor_size, r.n_lights), i
            assert np.array_equal(np.array(g.kpts, np.float32), np.array(r.kpts, np.float32) + np.tile(np.array(org, np.float32), 4)), i
            assert bytes(g.rvec) == bytes(r.rvec) and bytes(g.tvec) == bytes(r.tvec) and bytes(g.quat) == bytes(r.quat), i
            assert np.array_equal(np.array(g.xyxy, np.float32), boxes[i])
            n += g.pnp_ok
        assert n >= 3
        assert np.array_equal(w.get_rotated_image(), oracle.rotate180(crop))
        assert np.array_equal(p.get_rotated_image(), oracle.rotate180(crop))


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_on_a_live_engine(wblob):
    with peng(wblob) as p:
        assert p._L.irmv_engine_set_window(p._h, 0, 0, 0) == capi.ERR_ARG and b"no window" in p._L.irmv_last_error()
        assert p._L.irmv_engine_get_window(p._h, 0, None, None, None, None) == capi.ERR_ARG
        with pytest.raises(capi.IrmvError):
            p.set_window_center(10, 10)
    with weng(wblob, num_slots=2) as w:
        L, h = w._L, w._h
        for x0, y0 in [(-1, 0), (0, -1), (67, 0), (0, 74)]:          # one pixel outside the frame on each side
            assert L.irmv_engine_set_window(h, 0, x0, y0) == capi.ERR_ARG and b"inside" in L.irmv_last_error()
        for slot in (-1, 2):
            assert L.irmv_engine_set_window(h, slot, 0, 0) == capi.ERR_ARG and b"slot" in L.irmv_last_error()
            assert L.irmv_engine_get_window(h, slot, None, None, None, None) == capi.ERR_ARG
        assert L.irmv_engine_set_window(h, 1, 66, 73) == capi.OK     # the extreme that is inside
        assert w.window(1) == (66, 73, 256, 128) and w.window(0) == (33, 36, 256, 128)   # the refused calls changed nothing
