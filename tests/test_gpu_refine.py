"""The refined point source on the GPU (IRMV_POINTS_REFINED, irmv_engine_refine_points; k_light.hip's guided instantiation).

Every case predicts its result on the CPU first -- the guided extraction composed from the oracle's own building blocks plus
irmv_detection_amd.refine (tests/refine_craft.py) --, states how many of its records are refined, asserts that number on the
prediction and then on the GPU: points and flags bit for bit, poses to the bar tests/test_gpu_pnp.py holds irmv_pnp_solve to
(pnp_ref), with pnp_ok == 1 asserted wherever a pose is compared.

256 x 128 source pixels into a 128 x 64 net (exactly 2 : 1: the decode's fp32 arithmetic is exact, boxes and keypoints are
known in closed form); the window cases use tests/test_gpu_window.py's 322 x 201 frame with that window.

Step against hook: a not-refined record of a step is held byte for byte to the keypoint engine's record (whose pose comes
from the NMS kernel's lane-pair solver); the hook's own pose of its inputs comes from the scalar solver and is compared
where the step's does too: on refined records.
"""
import subprocess

import numpy as np
import pytest

import detect_craft as dc
import pnp_ref as P
import refine_craft as rc
from conftest import D_REF, K_REF
from irmv_detection_amd import capi, refine, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle

pytestmark = pytest.mark.gpu

SRC, NET, FULL, WIN = rc.SRC, rc.NET, rc.FULL, rc.WIN
KP, HEAD, CLASSICAL, REFINED = capi.POINTS_KEYPOINT_HEAD, capi.POINTS_KEYPOINT_HEAD, capi.POINTS_CLASSICAL, capi.POINTS_REFINED
NL, RS = capi.Det.n_lights.offset, capi.Det.reserved.offset
f32 = np.float32


@pytest.fixture(scope="module")
def sblob(blob):
    return rc.step_blob(blob)


def eng(blob, source, size=SRC, **kw):
    return YoloEngine(None, size, weights_blob=blob, net_size=NET[0], net_height=NET[1], point_source=source, **kw)


def raw(d, mask=(NL, RS)):
    """The record's bytes with the fields at the given offsets zeroed."""
    b = bytearray(bytes(d))
    for off in mask:
        b[off:off + 4] = b"\0\0\0\0"
    return bytes(b)


def kp(d):
    return np.array(d.kpts, f32)


def pose(d):
    return np.concatenate([np.array(d.rvec), np.array(d.tvec), np.array(d.quat)]).tobytes()


def head_with(e, recs):
    """A head with the given detections and nothing else.  recs: (ix, iy, (l, t, r, b) in strides, logit, kpts [8] in source
    pixels) on the stride-8 level; the box is ((ix + .5 - l) 8, ..) in net pixels = twice that in source pixels; the
    keypoint columns are v = (k_net / 8 - (ix, iy)) / 2 with k_net = k_src / 2: dyadic, exact."""
    A, no = e.num_anchors, e.head_channels
    nc = no - 64 - 8
    h = np.zeros((A, no), f32)
    h[:, :64] = dc.dfl_bias(0)
    h[:, 64:64 + nc] = dc.DARK
    for n, (ix, iy, sides, logit, k) in enumerate(recs):
        a = iy * (NET[0] // 8) + ix
        for j, d in enumerate(sides):
            h[a, 16 * j:16 * j + 16] = dc.OFF_BIN
            h[a, 16 * j + int(d)] = 0.0
            if d != int(d):
                h[a, 16 * j + int(d) + 1] = 0.0
        h[a, 64 + 3] = f32(logit)
        kn = np.asarray(k, np.float64).reshape(4, 2) / 2.0
        h[a, 64 + nc:] = ((kn / 8.0 - [ix, iy]) / 2.0).reshape(8)
    return h


def box_of(ix, iy, sides):
    l, t, r, b = sides
    return np.array([(ix + .5 - l) * 16, (iy + .5 - t) * 16, (ix + .5 + r) * 16, (iy + .5 + b) * 16], f32)


def post(e, img, head, rot=True):
    """The frame into the slot's device frame (a whole step), then the crafted head through run_post."""
    e.get_src_image_buffer()[:] = rc.to_buffer(img, rot)
    e.detect()
    e.write_head(head, 0)
    e.run_post(0, 1)
    return e.results_raw(0)


def check_pose(d, size=0, K=K_REF, D=D_REF):
    """The record's pose against the mpmath reference of the points it reports, to pnp_ref's bar."""
    assert d.pnp_ok == 1
    pts = kp(d)
    a = P.solve64(K, D, pts, size)
    b = P.solve_mp(K, D, pts, size, hnull=a["hnull"])
    c = P.classify(a, b)
    assert not c["degenerate"] and b["ok"]
    passed, err, which = P.check(P.matrix_of(np.array(d.rvec)), np.array(d.tvec), True, b, c)
    assert passed, (err, c["bar"])
    q, qr = np.array(d.quat), P.quat_of(b["R"][which])
    assert min(np.abs(q - qr).max(), np.abs(q + qr).max()) <= c["bar"]
    return err


def same_as_prediction(recs, pred, origin=(0.0, 0.0)):
    o8 = np.tile(np.array(origin, f32), 4)
    assert len(recs) == len(pred)
    for i, (d, p) in enumerate(zip(recs, pred)):
        assert (d.reserved, d.n_lights) == (p["flag"], p["n_lights"]), (i, d.reserved, d.n_lights, p["flag"], p["n_lights"])
        assert np.array_equal(kp(d), p["kpts"] + o8), (i, kp(d), p["kpts"])
        assert d.armor_valid == 1
        if p["flag"] == 1:
            assert d.pnp_ok == 1, i


def step_equals_hook(rd, kd, hk):
    """A refined engine's records against the keypoint engine's records and the hook's output on them, field for field."""
    assert len(rd) == len(kd)
    for i, (r, k) in enumerate(zip(rd, kd)):
        h = hk[i]
        assert (r.reserved, r.n_lights) == (h.reserved, h.n_lights), i
        assert np.array_equal(kp(r), kp(h)), i
        assert (tuple(r.xyxy), r.score, r.class_id, r.anchor, r.armor_valid, r.armor_size) == (tuple(k.xyxy), k.score, k.class_id, k.anchor, k.armor_valid, k.armor_size), i
        assert (h.armor_valid, h.armor_size) == (1, r.armor_size)
        assert k.reserved == 0 and k.n_lights == 0
        if r.reserved == 1:
            assert r.pnp_ok == 1 and h.pnp_ok == 1 and pose(r) == pose(h), i
        else:
            assert raw(r) == raw(k), i                       # the head's record, untouched
            assert np.array_equal(kp(h), kp(k)) and h.pnp_ok == k.pnp_ok, i


def inputs_of(recs):
    return np.array([list(d.xyxy) for d in recs], f32).reshape(-1, 4), np.array([list(d.kpts) for d in recs], f32).reshape(-1, 8)


# ---- 1. two bars with keypoints near them ---------------------------------------------------------------------------
PLATE1 = (6, 3, (2, 1, 2, 1))          # anchor and sides: box (72, 40, 136, 72), centre (104, 56)
OFF1 = np.array([(1.5, -2), (-1, 2.5), (2, 1), (-1.5, -3)], f32)   # keypoints 1 - 3 px off the bars' ends


def scene1():
    img = rc.blank()
    ends = rc.plate_bars(img, (104, 56))
    k = np.array([v for p in ends for v in p], f32) + OFF1.reshape(8)
    return img, box_of(*PLATE1), k, np.array([v for p in ends for v in p], f32)


@pytest.mark.parametrize("rot", [True, False])
def test_two_bars_near_the_keypoints(blob, rot):
    """Refined: 1 of 1.  The points are the bars' ends, the pose is theirs, the net's own keypoints stay the head's."""
    img, box, k, ends = scene1()
    pred = rc.predict(img, [box], [k], camera=(K_REF, D_REF))
    assert [p["flag"] for p in pred] == [1] and np.array_equal(pred[0]["kpts"], ends) and pred[0]["n_lights"] == 2
    assert ends.tolist() == [83.5, 67, 83.5, 44, 124.5, 44, 124.5, 67]
    with eng(blob, HEAD, rotate180=rot) as K, eng(blob, REFINED, rotate180=rot) as R:
        assert (K.point_source, R.point_source) == (HEAD, REFINED) and R.get_refine() == (0.5, 4.0)
        head = head_with(K, [PLATE1[:2] + (PLATE1[2], 2.0, k)])
        kd, rd = post(K, img, head, rot), post(R, img, head, rot)
        assert len(kd) == len(rd) == 1
        assert np.array_equal(np.array(kd[0].xyxy, f32), box) and np.array_equal(kp(kd[0]), k) and kd[0].reserved == 0   # the closed form of the inputs
        same_as_prediction(rd, pred)
        assert sum(d.reserved == 1 for d in rd) == 1
        err = check_pose(rd[0])
        assert pose(rd[0]) != pose(kd[0]) and kd[0].pnp_ok == 1
        assert np.array_equal(R.read_raw(0)["kpts"], K.read_raw(0)["kpts"])          # irmv_raw_dets.det_kpts: the net's output
        assert bytes(rd[0])[:capi.Det.pnp_ok.offset] == bytes(kd[0])[:capi.Det.pnp_ok.offset]   # box, score, class, anchor: the head's
        print(f"rot={rot}: refined pose error {err:.3g} against the mpmath reference")


# ---- 2. four bars in one ROI -----------------------------------------------------------------------------------------
def test_four_bars_the_keypoints_choose_the_plate(blob):
    """Two plates side by side in one bbox, the keypoints on the second.  Refined: 1 of 1, with the second plate's bars.  The
    classical source pairs the two lights OpenCV's contour order puts in front -- here the FIRST plate's (found last) -- :
    a different quad on the same frame and box, which is what the refined source is for."""
    plate = (8, 3, (5.5, 1.5, 5.5, 1.5))                    # box (48, 32, 224, 80)
    img = rc.blank()
    a = rc.plate_bars(img, (96, 58))                         # first plate: two rows lower, so its bars are found last
    b = rc.plate_bars(img, (176, 56))
    ends_a, ends_b = (np.array([v for p in e for v in p], f32) for e in (a, b))
    k = ends_b + np.array([1, -1.5, 1, 2, -2, 1, -1, -2], f32)
    box = box_of(*plate)
    pred = rc.predict(img, [box], [k], camera=(K_REF, D_REF))
    assert [p["flag"] for p in pred] == [1] and pred[0]["n_lights"] == 4 and np.array_equal(pred[0]["kpts"], ends_b)
    o = oracle.extract_armor(img, box)
    assert o["n_lights"] == 4 and (not o["ok"] or not np.array_equal(o["pts"].reshape(8), ends_b))
    with eng(blob, REFINED) as R, eng(blob, CLASSICAL) as Cl:
        head = head_with(R, [plate[:2] + (plate[2], 2.0, k)])
        rd, cd = post(R, img, head), post(Cl, img, head)
        assert len(rd) == len(cd) == 1 and np.array_equal(np.array(cd[0].xyxy, f32), box)
        same_as_prediction(rd, pred)
        assert sum(d.reserved == 1 for d in rd) == 1
        check_pose(rd[0])
        assert cd[0].n_lights == 4 and cd[0].armor_valid == (1 if o["ok"] else 0) and cd[0].reserved == 0
        assert np.array_equal(kp(cd[0]), o["pts"].reshape(8) if o["ok"] else np.zeros(8, f32))
        assert not np.array_equal(kp(cd[0]), kp(rd[0]))     # the feature's reason
        if o["ok"]:
            assert np.array_equal(kp(cd[0]), ends_a)
        # the classical instantiation is intact on a refined engine too
        assert raw(R.extract_armors_raw([box])[0], ()) == raw(Cl.extract_armors_raw([box])[0], ())


# ---- 3. fallbacks ---------------------------------------------------------------------------------------------------
def test_fallbacks_keep_the_heads_record(blob):
    """Four detections: keypoints beyond snap, one bar missing, both keypoint pairs at one bar, and one that refines.
    Refined: 1 of 4.  The other three are the keypoint engine's records byte for byte, apart from n_lights and the flag."""
    anchors = [(3, 2), (11, 2), (3, 6), (11, 5)]
    sides = (2, 1, 2, 1)
    img = rc.blank()
    ks = []
    c = [((ix + .5) * 16, (iy + .5) * 16) for ix, iy in anchors]
    e0 = rc.plate_bars(img, c[0])
    ks.append(np.array([v for p in e0 for v in p], f32) + np.array([0, 13, 0, 13, 0, 13, 0, 13], f32))        # 2 * 169 > 0.25 * 529
    e1 = rc.plate_bars(img, c[1], which="R")
    ks.append((np.array(c[1], f32) + rc.QUAD).reshape(8))
    e2 = rc.plate_bars(img, c[2], which="L")
    one = np.array([e2[0][0], e2[0][1], e2[1][0], e2[1][1]], f32)
    ks.append(np.concatenate([one + [-1, 1, -1, -1], (one + [1, 1, 1, -1])[[2, 3, 0, 1]]]).astype(f32))       # LB, LT left of the bar; RT, RB right of it
    e3 = rc.plate_bars(img, c[3])
    ks.append(np.array([v for p in e3 for v in p], f32) + np.array([1, 1, -1, 2, 1, -1, 2, 1], f32))
    boxes = [box_of(ix, iy, sides) for ix, iy in anchors]
    pred = rc.predict(img, boxes, ks, camera=(K_REF, D_REF))
    assert [p["flag"] for p in pred] == [0, 0, 0, 1] and [p["n_lights"] for p in pred] == [2, 1, 1, 2]
    assert refine.select(pred[2]["lights"], ks[2], 0.5) == (False, 0, 0)               # one light for both sides
    assert refine.select(pred[0]["lights"], ks[0], 0.5) == (False, None, None)
    with eng(blob, HEAD) as K, eng(blob, REFINED) as R:
        head = head_with(K, [(ix, iy, sides, 3.0 - 0.25 * n, ks[n]) for n, (ix, iy) in enumerate(anchors)])
        kd, rd = post(K, img, head), post(R, img, head)
        assert len(kd) == len(rd) == 4
        for n in range(4):
            assert np.array_equal(kp(kd[n]), ks[n]) and np.array_equal(np.array(kd[n].xyxy, f32), boxes[n])
        same_as_prediction(rd, pred)
        assert [d.reserved for d in rd] == [0, 0, 0, 1]
        for n in range(3):
            assert raw(rd[n]) == raw(kd[n]) and kd[n].pnp_ok == 1
        check_pose(rd[3])
        assert raw(rd[3]) != raw(kd[3])


# ---- 4. no answer ---------------------------------------------------------------------------------------------------
def test_pool_exhaustion_is_no_answer(sblob):
    """Ten full-frame boxes through the hook: seven padded label images fit the pool (8 frame areas), the last three get no
    answer: flag -1, the input points kept.  Refined: 4 of 10 (plates 0, 1, 4, 5 of the step scene, found in the whole frame)."""
    img, _ = rc.step_scene()
    _, k8 = rc.step_detections()
    kpts = np.stack([k8[i % 8] for i in range(10)])
    boxes = np.tile(np.array([0, 0, SRC[0], SRC[1]], f32), (10, 1))
    pred = rc.predict(img, boxes, kpts, camera=(K_REF, D_REF))
    assert [p["flag"] for p in pred] == [1, 1, 0, 0, 1, 1, 0, -1, -1, -1]
    assert refine.label_bytes(SRC[0], SRC[1]) * 7 <= rc.label_pool(*SRC) < refine.label_bytes(SRC[0], SRC[1]) * 8
    with eng(sblob, HEAD) as K:
        K.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        out, tr = K.refine_points(boxes, kpts, trace=True)
        out = [out[i] for i in range(10)]
        same_as_prediction(out, pred)
        for i, p in enumerate(pred):
            assert (tr[i].pool_fit, tr[i].pool_offset, tr[i].label_pool) == (int(p["flag"] != -1), p["pool_offset"], rc.label_pool(*SRC)), i
            assert (tr[i].rx, tr[i].ry, tr[i].rw, tr[i].rh) == p["roi"] == (0, 0, SRC[0], SRC[1])
            if p["flag"] == -1:
                assert np.array_equal(kp(out[i]), kpts[i]) and out[i].n_lights == 0 and tr[i].too_large == 1
            else:
                assert tr[i].n_contours == 14 and out[i].n_lights == 13     # every bar of the frame; the plain 3 x 3 blob is a contour, not a light
        assert sum(d.reserved == 1 for d in out) == 4 and sum(d.reserved == -1 for d in out) == 3
        assert K.point_source == HEAD


# ---- 5. margin ------------------------------------------------------------------------------------------------------
def test_the_margin_keeps_a_bar_whole(blob):
    """Bottom keypoints 2 px inside the bars' ends and a bbox smaller still: with the default margin the bars are whole
    (refined, 1 of 1, the bars' ends); with margin 0 the ROI ends at the keypoints, cuts the bars, and the extraction
    measures the stumps (refined, 1 of 1, with the stumps' ends) -- as the prediction says."""
    img = rc.blank()
    ends = np.array([v for p in rc.plate_bars(img, (104, 56)) for v in p], f32)
    k = ends + np.array([-1.5, -2, -1.5, -2, 2.5, -2, 2.5, -2], f32)  # 2 px up, 1.5 / 2.5 px outward: (82, 65) (82, 42) (127, 42) (127, 65)
    box = np.array([92, 50, 116, 62], f32)
    whole = rc.predict(img, [box], [k], camera=(K_REF, D_REF))
    cut = rc.predict(img, [box], [k], margin=0.0, camera=(K_REF, D_REF))
    assert whole[0]["flag"] == 1 and np.array_equal(whole[0]["kpts"], ends)
    assert cut[0]["roi"] == (82, 42, 45, 23)                    # columns 82 .. 126, rows 42 .. 64: the last three rows of both bars are cut off
    assert cut[0]["flag"] == 1 and cut[0]["kpts"].tolist() == [83.5, 64, 83.5, 44, 124.5, 44, 124.5, 64]     # the stumps' ends
    with eng(blob, HEAD) as K:
        K.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        a, ta = K.refine_points([box], [k], trace=True)
        same_as_prediction([a[0]], whole)
        assert a[0].reserved == 1 and (ta[0].rx, ta[0].ry, ta[0].rw, ta[0].rh) == whole[0]["roi"]
        check_pose(a[0])
        K.set_refine(0.5, 0.0)
        b, tb = K.refine_points([box], [k], trace=True)
        same_as_prediction([b[0]], cut)
        assert (tb[0].rx, tb[0].ry, tb[0].rw, tb[0].rh) == cut[0]["roi"]
        assert b[0].reserved == 1
        check_pose(b[0])


# ---- 6. step against hook -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["graph", "eager"])
def test_step_equals_keypoint_step_plus_hook(sblob, form, monkeypatch):
    """A whole step through the crafted blob on the eight-plate scene.  Refined: 4 of 8."""
    monkeypatch.setenv("IRMV_SYNC_LAUNCH", form)
    img, want = rc.step_scene()
    boxes, kpts = rc.step_detections()
    pred = rc.predict(img, boxes, kpts, camera=(K_REF, D_REF))
    assert [p["flag"] for p in pred] == want and sum(want) == 4
    with eng(sblob, HEAD) as K, eng(sblob, REFINED) as R:
        assert R.sync_launch == form
        for e in (K, R):
            e.get_src_image_buffer()[:] = rc.to_buffer(img, True)
            e.detect()
        kd, rd = K.results_raw(0), R.results_raw(0)
        kb, kk = inputs_of(kd)
        assert np.array_equal(kb, boxes) and np.array_equal(kk, kpts)
        step_equals_hook(rd, kd, K.refine_points(kb, kk))
        same_as_prediction(rd, pred)
        assert sum(d.reserved == 1 for d in rd) == 4
        for d in rd:
            if d.reserved == 1:
                check_pose(d)
        names = [(o["name"], o["layer"]) for o in R.profile(0, 1)]
        assert ("light_refine", "refine_points") in names and all(o["name"] != "light_refine" for o in K.profile(0, 1))
        assert [d.reserved for d in R.results_raw(0)] == want                    # (the profile's step repeats nothing of the refinement)


def test_step_equals_hook_two_slots_batched(sblob):
    """Two slots in one batched step, the second frame with the scene's rows of plates exchanged.  Refined: 4 of 8 in each."""
    img, want = rc.step_scene()
    img2 = np.roll(img, 64, axis=0)
    want2 = want[4:] + want[:4]
    boxes, kpts = rc.step_detections()
    preds = [rc.predict(img, boxes, kpts), rc.predict(img2, boxes, kpts)]
    assert [p["flag"] for p in preds[0]] == want and [p["flag"] for p in preds[1]] == want2
    with eng(sblob, HEAD, num_slots=2) as K, eng(sblob, REFINED, num_slots=2) as R:
        for e in (K, R):
            e.get_src_image_buffer(0)[:] = rc.to_buffer(img, True)
            e.get_src_image_buffer(1)[:] = rc.to_buffer(img2, True)
            e.submit(0, 2)
            e.wait_slots(0, 2)
        for s in (1, 0):
            kd, rd = K.results_raw(s), R.results_raw(s)
            kb, kk = inputs_of(kd)
            step_equals_hook(rd, kd, K.refine_points(kb, kk, slot=s))
            same_as_prediction(rd, preds[s])
            assert sum(d.reserved == 1 for d in rd) == 4


def weng(blob, source, **kw):
    return YoloEngine(None, FULL, weights_blob=blob, net_size=NET[0], net_height=NET[1], window=WIN, point_source=source, **kw)


def frame_view_scene():
    """The eight plates as a window engine's frame view sees them (322 x 201 into 128 x 64: the quads scaled by 2.515625 and
    3.140625, closed form detect_craft.to_source) with a 5 px wide bar at every keypoint pair."""
    kn = (np.array([(16 + 32 * ix, 16 + 32 * iy) for iy in range(2) for ix in range(4)], f32)[:, None, :] + rc.QUAD[None] / f32(2)).reshape(8, 8)
    k = dc.to_source(kn.reshape(-1, 2), FULL, NET[0], NET[1]).reshape(8, 8)
    img = rc.blank(FULL)
    for q in k.reshape(8, 4, 2):
        for top, bot in ((q[1], q[0]), (q[2], q[3])):
            y0, y1 = int(round(float(top[1]))), int(round(float(bot[1])))
            rc.bar(img, int(round(float(top[0]))) - 2, y0, 5, y1 - y0 + 1)
    c = dc.to_source(np.array([(16 + 32 * ix, 16 + 32 * iy) for iy in range(2) for ix in range(4)], f32), FULL, NET[0], NET[1])
    return img, np.concatenate([c, c], 1).astype(f32), k.astype(f32)


def test_step_equals_hook_window_and_frame_view(sblob):
    """A window engine at the frame's bottom-right corner (refined: 4 of 8, the scene inside the window), then the same slot in
    the frame view on a frame with a bar at every keypoint pair (refined: 8 of 8)."""
    org = (FULL[0] - WIN[0], FULL[1] - WIN[1])
    big, want = rc.step_scene(FULL, org)
    boxes, kpts = rc.step_detections()
    pred = rc.predict(big[org[1]:, org[0]:], boxes, kpts)
    assert [p["flag"] for p in pred] == want
    fimg, fboxes, fk = frame_view_scene()
    fpred = rc.predict(fimg, fboxes, fk)
    assert [p["flag"] for p in fpred] == [1] * 8
    with weng(sblob, HEAD) as K, weng(sblob, REFINED) as R:
        for e in (K, R):
            e.set_window(*org)
            e.get_src_image_buffer()[:] = rc.to_buffer(big, True)
            e.detect()
        kd, rd = K.results_raw(0), R.results_raw(0)
        kb, kk = inputs_of(kd)
        assert np.array_equal(kk, rc.step_detections(org)[1])
        step_equals_hook(rd, kd, K.refine_points(kb, kk))
        same_as_prediction(rd, pred, org)
        assert sum(d.reserved == 1 for d in rd) == 4
        graphs = R.debug_graph_count()
        for e in (K, R):
            e.set_view("frame")
            e.get_src_image_buffer()[:] = rc.to_buffer(fimg, True)
            e.detect()
        kd, rd = K.results_raw(0), R.results_raw(0)
        kb, kk = inputs_of(kd)
        assert np.array_equal(kk, fk) and np.array_equal(kb, fboxes)
        step_equals_hook(rd, kd, K.refine_points(kb, kk))
        same_as_prediction(rd, fpred)
        assert sum(d.reserved == 1 for d in rd) == 8 and R.debug_graph_count() == graphs + 1


def test_tiled_step_records_are_the_slots_records(sblob):
    """Two tiles of one frame in one tiled step: each slot's records equal the keypoint engine's tiled step plus the hook, and
    the merged list's records are byte-identical to the slots', flag included.  Refined: 4 of 8 in the tile that holds the
    scene; the other tile's count is the prediction's."""
    org = (FULL[0] - WIN[0], FULL[1] - WIN[1])
    corners = [(0, 0), org]
    big, want = rc.step_scene(FULL, org)
    boxes, kpts = rc.step_detections()
    preds = [rc.predict(big[y:y + WIN[1], x:x + WIN[0]], boxes, kpts) for x, y in corners]
    assert [p["flag"] for p in preds[1]] == want
    n_other = sum(p["flag"] == 1 for p in preds[0])
    with weng(sblob, HEAD, num_slots=3) as K, weng(sblob, REFINED, num_slots=3) as R:
        for e in (K, R):
            e.set_tiles(corners, 1)
            for s in range(3):                                  # (the hook looks at a slot's own frame)
                e.get_src_image_buffer(s)[:] = rc.to_buffer(big, True)
            e.submit_tiles(0, 1, 2)
            e.wait_slots(1, 2)
        for t, cnr in enumerate(corners):
            kd, rd = K.results_raw(1 + t), R.results_raw(1 + t)
            kb, kk = inputs_of(kd)
            step_equals_hook(rd, kd, K.refine_points(kb, kk, slot=1 + t))
            same_as_prediction(rd, preds[t], cnr)
            assert sum(d.reserved == 1 for d in rd) == (n_other, 4)[t]
        recs, n_in = R.tile_results_raw(1)
        assert n_in == 16 and len(recs) >= 8
        seen = 0
        for r in recs:
            assert raw(r.det, ()) == raw(R.results_raw(1 + r.tile)[r.index], ())
            seen += r.det.reserved == 1
        assert seen >= 4


# ---- 7. live parameters ---------------------------------------------------------------------------------------------
def test_live_parameters(sblob):
    """set_refine between steps: snap 4 admits plate 3's cut bars (refined 5 of 8; plate 2's one bar now serves both sides and
    stays kept); back to the defaults: 4 of 8.  No graph is captured anew; a refused value changes nothing."""
    img, want = rc.step_scene()
    boxes, kpts = rc.step_detections()
    wide = rc.predict(img, boxes, kpts, snap=4.0)
    assert [p["flag"] for p in wide] == [1, 1, 0, 1, 1, 1, 0, 0]
    with eng(sblob, REFINED) as R:
        R.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        R.detect()
        assert [d.reserved for d in R.results_raw(0)] == want
        graphs = R.debug_graph_count()
        R.set_refine(4.0, 4.0)
        assert R.get_refine() == (4.0, 4.0)
        R.detect()
        same_as_prediction(R.results_raw(0), wide)
        for bad in ((0.0, 4.0), (float("nan"), 4.0), (0.5, 64.5), (0.5, -1.0), (4.5, 4.0)):
            with pytest.raises(capi.IrmvError) as ei:
                R.set_refine(*bad)
            assert ei.value.code == capi.ERR_ARG
        assert R.get_refine() == (4.0, 4.0)
        R.detect()
        same_as_prediction(R.results_raw(0), wide)
        R.set_refine()
        R.detect()
        assert [d.reserved for d in R.results_raw(0)] == want and R.debug_graph_count() == graphs


# ---- 8. the other point sources, side by side ----------------------------------------------------------------------------
def test_keypoint_and_classical_engines_beside_a_refined_one(sblob):
    """A keypoint and a classical engine created next to a refined one return what they return alone: the head's points with
    flag 0, and the classical extraction's result (the oracle's) on a box around plate 0."""
    img, _ = rc.step_scene()
    boxes, kpts = rc.step_detections()
    box = np.array([4, 12, 60, 52], f32)
    o = oracle.extract_armor(img, box)
    assert o["ok"] and o["n_lights"] == 2
    with eng(sblob, REFINED) as R, eng(sblob, HEAD) as K, eng(sblob, CLASSICAL) as Cl:
        for e in (R, K, Cl):
            e.get_src_image_buffer()[:] = rc.to_buffer(img, True)
            e.detect()
        kd, cd = K.results_raw(0), Cl.results_raw(0)
        assert (R.point_source, K.point_source, Cl.point_source) == (REFINED, HEAD, CLASSICAL)
        assert len(kd) == len(cd) == 8 and np.array_equal(inputs_of(kd)[1], kpts)
        assert all(d.reserved == 0 and d.n_lights == 0 and d.armor_valid == 1 and d.pnp_ok == 1 for d in kd)
        assert all(d.reserved == 0 and d.armor_valid == 0 for d in cd)          # point-like boxes hold no ROI
        for e in (K, Cl, R):
            a = e.extract_armors_raw([box])[0]
            assert a.armor_valid == 1 and np.array_equal(kp(a), o["pts"].reshape(8)) and a.n_lights == 2 and a.reserved == 0


def test_facade_runs_the_refined_engine(sblob, tmp_path):
    """The C++ facade's refined engine on the eight-plate scene: the flags and points of the Python mirror, before and after
    set_refine(0.75, 6)."""
    import test_refine
    exe = test_refine.facade_exe(build=False)
    img, want = rc.step_scene()
    (tmp_path / "m.irmw").write_bytes(sblob)
    (tmp_path / "frame.raw").write_bytes(rc.to_buffer(img, True).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "m.onnx"), str(tmp_path / "frame.raw")], text=True).splitlines()
    assert out[0] == "refines 1 keypoint_head 1"
    boxes, kpts = rc.step_detections()
    with eng(sblob, REFINED) as R:
        R.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        lines = []
        for p, par in enumerate(((0.5, 4.0), (0.75, 6.0))):
            R.set_refine(*par)
            R.detect()
            rd = R.results_raw(0)
            lines.append(f"pass {p} records {len(rd)}")
            for i, d in enumerate(rd):
                lines.append(f"det {i} flag {d.reserved} lights {d.n_lights} " + " ".join(f"{v:08x}" for v in kp(d).view(np.uint32)))
    assert out[1:] == lines and [int(l.split()[3]) for l in out[2:10]] == want
