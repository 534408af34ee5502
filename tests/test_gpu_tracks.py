"""Armor tracks on the GPU (k_track.hip): the stand-alone tracker on every scenario of tests/track_set.py, whole steps of every
launch form fed to the host reference (irmv_detection_amd/tracks.py) record by record, the submit-order contract, the switch,
and the memory classes.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import mem_residue as MR
import refine_craft as rc
import track_set as TS
from irmv_detection_amd import capi, frames, tracks as T, window
from irmv_detection_amd.engine import Tracker, YoloEngine
from test_gpu_window import FULL, K, NET, WIN, frame_of

pytestmark = pytest.mark.gpu

ZERO_DET = bytes(T.DET_TRACK_SIZE)
SCENARIOS = {sc["name"]: sc for sc in TS.scenarios()}


@pytest.fixture(scope="module")
def wblob(blob):
    return dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))


def peng(blob, src=WIN, **kw):
    kw.setdefault("camera_matrix", K)
    return YoloEngine(None, src, weights_blob=blob, net_size=NET[0], net_height=NET[1], **kw)


def put(e, frame, slot=0):
    e.get_src_image_buffer(slot)[:] = frame


def win_frame(i):
    return frames.synthetic_frame(i, WIN[0], WIN[1])


def opts_kw(o):
    return dict(confirm_hits=o.confirm_hits, max_misses=o.max_misses, match_class=o.match_class, gate=o.gate, max_coast_s=o.max_coast_s,
                accel_sigma=o.accel_sigma, init_vel_sigma=o.init_vel_sigma, sigma_lat=o.sigma_lat, sigma_rng=o.sigma_rng)


def got_bytes(dets, frame, snap):
    return b"".join(bytes(d) for d in dets), bytes(frame), b"".join(bytes(t) for t in snap)


def slot_bytes(e, slot=0):
    frame, snap = e.tracks(slot)
    return got_bytes(e.det_tracks(slot), frame, snap)


def step_obs(e, slot=0):
    """What a step reports, as the reference's observations: its irmv_det records, and their irmv_pose_cov where enabled."""
    dets = e.results_raw(slot)
    covs = e.pose_covs(slot) if e.pose_cov()["enable"] else [None] * len(dets)
    obs = []
    for d, c in zip(dets, covs):
        cov = None
        if c is not None and c.state == 1:
            cov = tuple(c.cov[T.POSE_COV_T[i][j]] for i in range(3) for j in range(3))
        obs.append(T.Obs(d.class_id, tuple(d.tvec), 1 if (d.pnp_ok == 1 and d.armor_valid == 1) else 0, cov))
    return obs


def check_step(ref, e, slot, t, Rw=T.IDENTITY, tw=(0.0, 0.0, 0.0)):
    """The slot's two records against the reference tracker fed the step's own records -> (det_tracks, frame, snapshot)."""
    res = ref.update(t, step_obs(e, slot), Rw, tw)
    want, got = TS.pack_result(res), slot_bytes(e, slot)
    assert got[1] == want[1], (slot, t, e.tracks(slot)[0].state, res[1])
    assert got[0] == want[0] and got[2] == want[2], (slot, t)
    return res


# ---- 1. the stand-alone tracker --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_tracker_equals_the_reference_on_every_scenario(name):
    """Frame by frame: the detection records, the frame header and the 32-track snapshot, bit for bit.  ("sizes" brings frames
    of 0, 1, 2, 33, 65 and 256 observations.)"""
    sc = SCENARIOS[name]
    want = TS.run_reference(sc)
    tr = Tracker(**opts_kw(sc["opts"]))
    try:
        for f, ((t, Rw, tw, obs), res) in enumerate(zip(sc["frames"], want)):
            got = tr.update(t, [(o.cls, o.tvec, o.valid, o.cov) for o in obs], Rw, tw)
            w, g = TS.pack_result(res), got_bytes(*got)
            assert g[1] == w[1], (name, f, "frame header")
            assert g[0] == w[0], (name, f, "detection records", next(i for i in range(len(obs)) if g[0][72 * i:72 * i + 72] != w[0][72 * i:72 * i + 72]))
            assert g[2] == w[2], (name, f, "snapshot", next(k for k in range(32) if g[2][384 * k:384 * k + 384] != w[2][384 * k:384 * k + 384]))
    finally:
        tr.close()


def test_tracker_reset_keeps_the_id_counter_and_objects_are_independent():
    a, b = Tracker(), Tracker(confirm_hits=1)
    try:
        ob = [(2, (0.1, 0.0, 3.0), 1, None)]
        d, f, s = a.update(1.0, ob)
        assert (d[0].state, d[0].id, f.next_id, s[0].state) == (T.DET_STARTED, 1, 2, T.TENTATIVE)
        d, f, s = b.update(1.0, ob)
        assert (d[0].id, s[0].state) == (1, T.CONFIRMED)
        a.reset()
        d, f, s = a.update(0.5, ob)                       # (an earlier stamp: the reset cleared the table's stamp too)
        assert (f.state, d[0].state, d[0].id, d[0].track, f.n_live) == (1, T.DET_STARTED, 2, 0, 1)
    finally:
        a.close()
        b.close()


# ---- 2. refusals on the device ----------------------------------------------------------------------------------------------
def test_a_refused_frame_writes_zero_records_and_nothing_beside_them():
    tr = Tracker()
    try:
        L, h = tr._L, tr._h
        obs = (capi.TrackObs * 3)()
        for i in range(3):
            obs[i].class_id, obs[i].valid = i, 1
            obs[i].tvec[:] = [0.3 * i, 0.0, 3.0]
        dets = (capi.DetTrack * 5)()
        frame, snap = capi.TrackFrame(), (capi.Track * 32)()
        capi.check(L.irmv_tracker_update(h, 2.0, None, None, obs, 3, dets, C.byref(frame), snap))
        first = bytes(snap)
        assert frame.state == 1 and frame.n_live == 3
        C.memset(dets, 0xA5, C.sizeof(dets))
        for stale in (2.0, 1.5, float("nan")):
            capi.check(L.irmv_tracker_update(h, stale, None, None, obs, 2, dets, C.byref(frame), snap))
            assert frame.state == -2 and frame.next_id == 4 and (frame.n_live, frame.n_started) == (0, 0)
            assert bytes(dets)[:144] == bytes(144) and bytes(dets)[144:] == b"\xa5" * 216      # two zero records, their neighbours untouched
            back = bytearray(bytes(snap))
            for k in range(32):
                assert snap[k].det == -1
                back[384 * k + 20:384 * k + 24] = first[384 * k + 20:384 * k + 24]
            assert bytes(back) == first                                                        # the table, but for the snapshot's det
        capi.check(L.irmv_tracker_update(h, 2.01, None, None, obs, 3, dets, C.byref(frame), snap))
        assert frame.state == 1 and [d.state for d in dets[:3]] == [1, 1, 1] and [d.hits for d in dets[:3]] == [2, 2, 2]
        assert L.irmv_tracker_update(h, 3.0, None, None, obs, 257, dets, None, None) == capi.ERR_ARG
        assert L.irmv_tracker_update(h, 3.0, None, None, None, 1, dets, None, None) == capi.ERR_ARG
        bad = (C.c_double * 9)(*([float("inf")] * 9))
        assert L.irmv_tracker_update(h, 3.0, bad, None, obs, 1, dets, None, None) == capi.ERR_ARG
    finally:
        tr.close()


# ---- 3. whole steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov", [False, True], ids=["cov-off", "cov-on"])
def test_one_frame_stepped_eight_times_then_a_translating_camera(wblob, cov):
    with peng(wblob) as e:
        n = C.c_int(0)
        assert e._L.irmv_engine_det_tracks(e._h, 0, (capi.DetTrack * e.max_det)(), e.max_det, C.byref(n)) == capi.ERR_ARG
        assert e.tracking()["enable"] == 0 and e.tracking()["gate"] == 16.27 and e.tracking()["confirm_hits"] == 3
        if cov:
            e.set_pose_cov(sigma_px=0.7)
        e.set_tracking()
        assert e.tracking()["enable"] == 1
        put(e, win_frame(22))                                            # 88 detections, all solved: more than the table holds
        ref = T.Tracker()
        started = {}
        for k in range(8):
            t = 1.0 + 0.01 * k
            e.set_stamp(t)
            assert e.stamp() == t
            e.detect()
            dets, frame, snap = check_step(ref, e, 0, t)
            assert frame.state == 1
            if k == 0:
                started = {i: d.id for i, d in enumerate(dets) if d.state == T.DET_STARTED}
                assert len(started) == 32 and frame.n_no_room >= 1 and frame.n_confirmed == 0
            else:
                for i, id_ in started.items():
                    assert (dets[i].state, dets[i].id, dets[i].d2, dets[i].hits) == (T.DET_MATCHED, id_, 0.0, k + 1)
                assert frame.n_confirmed == (32 if k >= 2 else 0) and frame.n_no_room >= 1
        assert cov == any(o.cov is not None for o in step_obs(e))
        # the camera moves 5 cm a step along x: the world positions move, the tracks follow with a velocity
        for k in range(8, 14):
            t = 1.0 + 0.01 * k
            tw = (0.05 * (k - 7), 0.0, 0.0)
            e.set_stamp(t)
            e.set_camera_pose(T.IDENTITY, tw)
            assert tuple(e.camera_pose()[1]) == tw
            e.detect()
            dets, frame, snap = check_step(ref, e, 0, t, T.IDENTITY, tw)
        assert any(d.state == T.DET_MATCHED and d.vel[0] > 0.5 for d in dets)


def test_a_window_engine_whose_window_moves_and_its_frame_view(wblob):
    frame = frame_of(16)
    with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, camera_matrix=K) as w:
        w.set_pose_cov(sigma_px=0.7)
        w.set_tracking(max_misses=2)
        put(w, frame)
        ref = T.Tracker(T.Options(max_misses=2))
        seen = set()
        for k, org in enumerate(((3, 70), (3, 70), (5, 68), (60, 2), (60, 2), "frame", "frame")):
            if org == "frame":
                w.set_view("frame")
            else:
                w.set_window(*org)
            w.set_stamp(0.5 + 0.02 * k)
            w.detect()
            dets, fr, _ = check_step(ref, w, 0, 0.5 + 0.02 * k)
            seen |= {d.state for d in dets}
        assert {T.DET_MATCHED, T.DET_STARTED} <= seen


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_classical_and_refined_point_sources(blob, source):
    """The eight-plate scene of the refined tests as whole steps: the tracker reads the records the light extraction wrote."""
    sblob = rc.step_blob(blob)
    img, _ = rc.step_scene()
    with YoloEngine(None, rc.SRC, weights_blob=sblob, net_size=rc.NET[0], net_height=rc.NET[1], point_source=source) as e:
        e.set_tracking()
        put(e, rc.to_buffer(img, True))
        ref = T.Tracker()
        for k in range(4):
            e.set_stamp(0.1 * (k + 1))
            e.set_camera_pose(T.IDENTITY, (0.0, 0.01 * k, 0.0))
            e.detect()
            dets, frame, _ = check_step(ref, e, 0, 0.1 * (k + 1), T.IDENTITY, (0.0, 0.01 * k, 0.0))
        assert len(e.results_raw(0)) >= 4
        assert source == capi.POINTS_CLASSICAL or (frame.n_confirmed >= 4 and sum(d.state == T.DET_MATCHED for d in dets) >= 4)


def test_classical_engine_on_the_one_plate_frames(blob):
    """The frames of tests/test_gpu_side_records.py: the seeded step frames with one plate's two bars drawn in, binary threshold
    250 -- whole steps of a classical engine that solve an armor -- stepped through three seeds twice, the camera translating,
    with the pose covariance on."""
    import test_gpu_patches as TP
    import test_gpu_side_records as SR
    with TP.eng(blob, point_source=capi.POINTS_CLASSICAL, binary_threshold=250) as e:
        e.set_pose_cov(sigma_px=0.7)
        e.set_tracking()
        ref = T.Tracker()
        solved = matched = 0
        for k in range(6):
            TP.put(e, SR.barred(k % 3), True)
            tw = (0.02 * k, 0.0, 0.0)
            e.set_stamp(2.0 + 0.01 * k)
            e.set_camera_pose(T.IDENTITY, tw)
            e.detect()
            dets, frame, _ = check_step(ref, e, 0, 2.0 + 0.01 * k, T.IDENTITY, tw)
            solved += sum(d.state != T.DET_NONE for d in dets)
            matched += sum(d.state == T.DET_MATCHED for d in dets)
        assert solved >= 6 and matched >= 1 and frame.n_live >= 1


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------
def test_tracks_advance_in_submit_order_on_any_grouping(wblob):
    """Three slots on two streams.  Each sequence of submits, with no wait between them, gives every slot the records of a
    one-slot engine stepped synchronously through the same frames and stamps in the sequence's order; a stale stamp in the
    middle is refused and the steps around it are as if it had not been."""
    fr = [win_frame(20 + i) for i in range(3)]
    sequences = [[(0, 1), (1, 1), (2, 1)], [(0, 3)], [(1, 2), (0, 1)], [(2, 1), (0, 2)]]
    with peng(wblob) as one, peng(wblob, num_slots=3, num_streams=2) as e:
        for x in (one, e):
            x.set_tracking(max_misses=1)
        for s in range(3):
            put(e, fr[s], s)
        t = 1.0
        for seq in sequences + ["stale"]:
            stale = seq == "stale"
            order = [s for f, c in (sequences[0] if stale else seq) for s in range(f, f + c)]
            stamps = {}
            for s in order:
                t += 0.01
                stamps[s] = t
            if stale:
                stamps[order[1]] = stamps[order[0]] - 0.005
            for x in (one, e):
                x.wait()
                x.reset_tracks()
            want = {}
            for s in order:
                if stale and s == order[1]:
                    continue
                put(one, fr[s])
                one.set_stamp(stamps[s])
                one.detect()
                want[s] = (slot_bytes(one), [bytes(d) for d in one.results_raw(0)])
            for s in order:
                e.set_stamp(stamps[s], s)
            for f, c in (sequences[0] if stale else seq):
                e.submit(f, c)
            e.wait()
            for s in order:
                if stale and s == order[1]:
                    frame, snap = e.tracks(s)
                    assert frame.state == -2 and frame.stamp == stamps[s]
                    assert all(bytes(d) == ZERO_DET for d in e.det_tracks(s)) and len(e.det_tracks(s)) == len(e.results_raw(s))
                    continue
                assert [bytes(d) for d in e.results_raw(s)] == want[s][1], (seq, s)
                assert slot_bytes(e, s) == want[s][0], (seq, s)
            assert e.tracks(order[-1])[0].n_live >= 1
        assert one.tracks(0)[0].next_id == e.tracks(order[-1])[0].next_id > 1


# ---- 5. enable, disable, reset ------------------------------------------------------------------------------------------------
def _everything(e, slot=0):
    return dict(dets=[bytes(d) for d in e.results_raw(slot)], yaws=[bytes(y) for y in e.yaw_poses(slot)], covs=[bytes(c) for c in e.pose_covs(slot)])


def test_enable_disable_reset_and_the_steps_that_do_not_feed(wblob):
    frame = frame_of(12)

    def mk(on):
        e = YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, num_slots=3, camera_matrix=K)
        e.set_yaw_solve()
        e.set_pose_cov(sigma_px=0.7)
        for s in range(3):
            put(e, frame, s)
        e.detect(0)
        return e

    with mk(False) as never, mk(True) as e:
        g0 = e.debug_graph_count()
        e.set_tracking()
        assert e.debug_graph_count() == g0                               # nothing re-captured
        ref = T.Tracker()
        t = 1.0
        for k in range(3):
            t += 0.01
            e.set_stamp(t)
            e.detect(0)
            check_step(ref, e, 0, t)
        assert e.debug_graph_count() == g0
        never.detect(0)
        assert _everything(e) == _everything(never) and len(_everything(e)["dets"]) >= 1   # the other channels do not notice
        for x in (never, e):
            x.submit(0, 3)
            x.wait()
        for s in range(3):
            assert _everything(e, s) == _everything(never, s)
        for s in range(3):                                               # (all three slots carried stamp <= t: slot 0's, then 0 and 0)
            assert e.tracks(s)[0].state == -2
        # a tiled step and run_post leave the table alone and their slots' channels zero
        before = slot_bytes(e, 0)
        e.set_tiles([(0, 0), (66, 73)], 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        e.run_post(0, 1)
        for s in range(3):
            d, f, sn = slot_bytes(e, s)
            assert not any(d) and not any(f) and not any(sn), s
        t += 0.01
        e.set_stamp(t)
        e.detect(0)
        res = check_step(ref, e, 0, t)                                   # the reference never saw the tiled step or run_post
        assert res[1].n_confirmed >= 1
        next_id = res[1].next_id
        # reset_tracks: the table only
        kept = slot_bytes(e, 0)
        e.reset_tracks()
        assert slot_bytes(e, 0) == kept
        ref.reset()
        e.set_stamp(0.25)                                                # (the stamp went with the table)
        e.detect(0)
        res = check_step(ref, e, 0, 0.25)
        assert res[1].state == 1 and res[1].n_confirmed == 0 and min(d.id for d in res[0] if d.state == T.DET_STARTED) == next_id
        # disable: both channels zero at once, no step writes them, the table is cleared, the ids go on
        next_id = res[1].next_id
        g1 = e.debug_graph_count()                                       # (the batched, tiled and post steps above captured theirs)
        e.set_tracking(enable=False)
        assert not any(b"".join(slot_bytes(e, 0)))
        e.detect(0)
        assert not any(b"".join(slot_bytes(e, 0))) and e.debug_graph_count() == g1
        e.set_tracking()
        assert not any(b"".join(slot_bytes(e, 0))) and e.debug_graph_count() == g1
        ref.reset()
        e.set_stamp(0.125)
        e.detect(0)
        res = check_step(ref, e, 0, 0.125)
        assert res[1].n_started >= 1 and min(d.id for d in res[0] if d.state == T.DET_STARTED) == next_id
        with pytest.raises(capi.IrmvError):
            e.set_tracking(gate=float("nan"))
        assert e.tracking()["gate"] == 16.27 and e.tracking()["enable"] == 1
        never.detect(0)
        assert _everything(e) == _everything(never)


# ---- 6. memory residue and classes ----------------------------------------------------------------------------------------
def test_records_do_not_depend_on_what_device_memory_held(wblob):
    def go(fill):
        with peng(wblob) as e:
            e.set_pose_cov(sigma_px=0.7)
            e.set_tracking()
            cls = {r["name"]: r["cls"] for r in e.debug_allocs()}
            assert cls["track_table"] == "CARRIED" and cls["dettrack_dev"] == "SCRATCH" and cls["tracks_dev"] == "SCRATCH"
            assert cls["track_opts"] == "CONST" and cls["track_slots"] == "CONST"
            put(e, win_frame(12))
            out = []
            for k in range(3):
                if fill is not None:
                    assert e.debug_fill_mem(fill) > 0
                e.set_stamp(1.0 + 0.01 * k)
                e.detect()
                out.append(MR.freeze([e.results_raw(0), e.det_tracks(0), [e.tracks(0)[0]], e.tracks(0)[1]]))
            return out

    fresh = go(None)
    for pattern in MR.PATTERNS[1:]:
        assert go(pattern) == fresh
