"""Armor tracks on the CPU: irmv_detection_amd/tracks.py (the arithmetic k_track.hip follows) against an independent textbook
filter, the scenario properties of tests/track_set.py asserted on the reference itself, and the host-side parts of the ABI
(struct sizes, option refusals, irmv_track_predict)."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import track_set as TS
from conftest import ROOT
from irmv_detection_amd import _build, capi
from irmv_detection_amd import tracks as T


@pytest.fixture(scope="module")
def ref():
    """Every scenario's reference run, computed once."""
    return {sc["name"]: (sc, TS.run_reference(sc)) for sc in TS.scenarios()}


# ---- an independent filter: numpy matrices, np.linalg.inv, Joseph form; written apart from tracks.py ---------------------
class TextbookTracker:
    def __init__(self, o):
        self.o, self.tracks, self.t, self.next_id = o, [None] * 32, None, 1

    def step(self, t, obs, Rw, tw):
        o = self.o
        Rw = np.array(Rw).reshape(3, 3)
        H = np.hstack([np.eye(3), np.zeros((3, 3))])
        if self.t is not None:
            dt = t - self.t
            F = np.eye(6)
            F[:3, 3:] = dt * np.eye(3)
            G = np.vstack([0.5 * dt * dt * np.eye(3), dt * np.eye(3)])
            Q = o.accel_sigma ** 2 * G @ G.T
            for tr in self.tracks:
                if tr:
                    tr["x"] = F @ tr["x"]
                    tr["P"] = F @ tr["P"] @ F.T + Q
        meas = []
        for ob in obs:
            tv = np.array(ob.tvec)
            if ob.valid != 1 or not np.all(np.isfinite(tv)) or tv[2] <= 0:
                meas.append(None)
                continue
            Cc = np.array(ob.cov).reshape(3, 3) if ob.cov is not None else np.diag([(o.sigma_lat * tv[2]) ** 2, (o.sigma_lat * tv[2]) ** 2, (o.sigma_rng * tv[2] ** 2) ** 2])
            Rn = Rw @ Cc @ Rw.T
            z = Rw @ tv + np.array(tw)
            meas.append((z, Rn) if np.all(np.isfinite(Rn)) and np.all(np.diag(Rn) > 0) else None)
        cand = []
        for k, tr in enumerate(self.tracks):
            for i, m in enumerate(meas):
                if tr and m and (o.match_class == 0 or obs[i].cls == tr["cls"]):
                    y = m[0] - H @ tr["x"]
                    d2 = float(y @ np.linalg.inv(H @ tr["P"] @ H.T + m[1]) @ y)
                    if d2 <= o.gate:
                        cand.append((d2, k, i))
        used_t, used_o = {}, {}
        for d2, k, i in sorted(cand):
            if k not in used_t and i not in used_o:
                used_t[k], used_o[i] = i, k
        for k, tr in enumerate(self.tracks):
            if not tr:
                continue
            if k in used_t:
                z, Rn = meas[used_t[k]]
                S = H @ tr["P"] @ H.T + Rn
                K = tr["P"] @ H.T @ np.linalg.inv(S)
                tr["x"] = tr["x"] + K @ (z - H @ tr["x"])
                A = np.eye(6) - K @ H
                tr["P"] = A @ tr["P"] @ A.T + K @ Rn @ K.T
                tr["hits"] += 1
                tr["misses"], tr["last"] = 0, t
                if tr["hits"] >= o.confirm_hits:
                    tr["state"] = 2
            else:
                tr["misses"] += 1
                if tr["misses"] > o.max_misses or t - tr["last"] > o.max_coast_s:
                    self.tracks[k] = None
        for i, m in enumerate(meas):
            if m and i not in used_o and None in self.tracks:
                k = self.tracks.index(None)
                P = np.zeros((6, 6))
                P[:3, :3], P[3:, 3:] = m[1], o.init_vel_sigma ** 2 * np.eye(3)
                self.tracks[k] = dict(id=self.next_id, cls=obs[i].cls, state=1, hits=1, misses=0, last=t, x=np.concatenate([m[0], np.zeros(3)]), P=P)
                self.next_id += 1
        self.t = t


def test_reference_agrees_with_an_independent_textbook_filter(ref):
    """Ids and life-cycle states identical; x and P within eight times the largest relative difference measured over the set
    (4.95e-14, DESIGN.md section 32: the simple and the Joseph update differ by rounding only), far below the 1e-9 at which one of
    the two would be wrong."""
    worst = 0.0
    for name in ("single_200", "three_200", "three_cov_60"):
        sc, res = ref[name]
        tb = TextbookTracker(sc["opts"])
        for (t, Rw, tw, obs), (_, frame, snap) in zip(sc["frames"], res):
            tb.step(t, obs, Rw, tw)
            for k, tr in enumerate(snap):
                o = tb.tracks[k]
                assert (tr.state != T.FREE) == (o is not None), (name, t, k)
                if o is None:
                    continue
                assert (tr.id, tr.state, tr.hits, tr.misses, tr.cls) == (o["id"], o["state"], o["hits"], o["misses"], o["cls"]), (name, t, k)
                x, P = np.array(tr.x), np.array(tr.P)
                worst = max(worst, float(np.max(np.abs(x - o["x"])) / np.max(np.abs(o["x"]))), float(np.max(np.abs(P - o["P"])) / np.max(np.abs(o["P"]))))
    print("largest relative difference to the textbook filter:", worst)
    assert worst <= 8 * 4.95e-14
    assert worst <= 1e-9


# ---- scenario properties, on the reference itself ---------------------------------------------------------------------------
def _ids(res):
    return [[d.id for d in dets] for dets, _, _ in res]


def test_crossing_targets_of_different_classes_keep_their_ids(ref):
    _, res = ref["crossing_mc1"]
    ids = _ids(res)
    assert all(i == ids[0] for i in ids) and ids[0][0] != ids[0][1]
    assert all(d.state == T.DET_MATCHED for dets, _, _ in res[1:] for d in dets)
    assert res[-1][1].n_confirmed == 2 and res[-1][1].n_live == 2


def test_crossing_with_match_class_off_follows_the_greedy_rule(ref):
    """With exact measurements on straight lines both filters predict well, so the nearest pair is each track's own target all
    the way through the crossing: the greedy rule keeps the ids here too, and no third track is ever started."""
    _, res = ref["crossing_mc0"]
    ids = _ids(res)
    assert ids == [ids[0]] * len(ids) and ids[0] == [1, 2]
    assert all(f.n_live == 2 and f.n_no_room == 0 for _, f, _ in res)
    assert res[-1][1].next_id == 3
    # what the rule gives at every frame: the least d2 first
    for dets, _, _ in res[1:]:
        assert all(d.state == T.DET_MATCHED and d.d2 <= 16.27 for d in dets)


def test_the_class_gate_decides_a_near_crossing(ref):
    """near_cross: the targets change sides between frames 0 and 1.  match_class = 1: every observation keeps the id of its class's
    track.  match_class = 0: the greedy rule takes the nearer pair first (1 cm, the other class's), and the ids swap for good."""
    _, on = ref["near_cross_mc1"]
    _, off = ref["near_cross_mc0"]
    assert _ids(on) == [[1, 2]] * 5
    assert _ids(off) == [[1, 2]] + [[2, 1]] * 4
    for res in (on, off):
        assert all(d.state == T.DET_MATCHED for dets, _, _ in res[1:] for d in dets) and res[-1][1].next_id == 3
    assert [t.cls for t in on[-1][2][:2]] == [1, 2] and [t.cls for t in off[-1][2][:2]] == [1, 2]     # a track keeps its birth class
    d_on, d_off = [d.d2 for d in on[1][0]], [d.d2 for d in off[1][0]]
    assert all(a > 10 * b > 0.0 for a, b in zip(d_on, d_off)) and max(d_on) < 16.27                    # 4 cm against 1 cm, both gated
    assert [TS.pack_result(r) for r in on] != [TS.pack_result(r) for r in off]


def test_a_track_is_deleted_after_max_coast_s_whatever_its_misses(ref):
    _, res = ref["coast"]
    _, never = ref["coast_never"]
    frames = [f for _, f, _ in res]
    assert [f.n_live for f in frames] == [1] * 9 + [0, 1] and [f.n_deleted for f in frames] == [0] * 9 + [1, 0]
    assert res[6][2][0].misses == 2 and res[7][0][0].state == T.DET_MATCHED and res[7][0][0].id == 1   # 0.4 s: kept, and matched
    assert res[8][2][0].misses == 1 and res[8][2][0].id == 1                                           # 0.3 s: kept
    assert res[9][2][0].state == T.FREE                                                                # 0.6 s, two misses of five
    assert res[10][0][0].state == T.DET_STARTED and res[10][0][0].id == 2
    # without the time limit the same frames keep the track: the branch, not the miss count, deleted it
    assert never[9][1].n_live == 1 and never[9][2][0].misses == 2 and never[10][0][0].id == 1 and never[10][0][0].state == T.DET_MATCHED


def test_dropout_of_max_misses_keeps_the_id_one_more_deletes(ref):
    _, keep = ref["dropout_5"]
    _, lose = ref["dropout_6"]
    assert keep[9][0][0].id == 1 and keep[15][0][0].id == 1 and keep[15][0][0].state == T.DET_MATCHED
    assert keep[14][1].n_live == 1 and keep[14][2][0].misses == 5
    assert lose[15][1].n_deleted == 1 and lose[15][1].n_live == 0
    assert lose[16][0][0].state == T.DET_STARTED and lose[16][0][0].id == 2


def test_forty_observations_give_32_tracks_and_8_no_room(ref):
    _, res = ref["crowd_40"]
    dets, frame, snap = res[0]
    assert (frame.n_live, frame.n_started, frame.n_no_room) == (32, 32, 8)
    assert [d.state for d in dets] == [T.DET_STARTED] * 32 + [T.DET_NO_ROOM] * 8
    assert all(d.track == -1 and d.id == 0 for d in dets[32:])
    dets, frame, _ = res[1]
    assert sum(d.state == T.DET_MATCHED for d in dets) == 32 and frame.n_no_room == 8 and frame.next_id == 33


def test_a_freed_entry_is_reused_at_the_lowest_index_with_a_fresh_id(ref):
    _, res = ref["free_reuse"]
    assert [t.id for t in res[3][2][:4]] == [1, 2, 3, 4]
    deleted_at = next(i for i, (_, f, _) in enumerate(res) if f.n_deleted)
    assert res[deleted_at][2][1].state == T.FREE and deleted_at < 16
    d = res[16][0][-1]
    assert (d.state, d.track, d.id) == (T.DET_STARTED, 1, 5)
    assert res[16][2][1].id == 5 and res[16][2][1].det == len(res[16][0]) - 1


def test_an_equal_distance_tie_goes_to_the_lower_observation(ref):
    sc, res = ref["tie"]
    dets = res[1][0]
    tr = T.Tracker(sc["opts"])
    tr.update(*[sc["frames"][0][i] for i in (0, 3, 1, 2)])
    x, P = T.predict(tr.tracks[0].x, tr.tracks[0].P, TS.DT, 8.0)
    d = []
    for ob in sc["frames"][1][3]:
        _, z, R = T.measure(ob, TS.EYE, TS.ZERO, sc["opts"])
        _, y, Si = T.innovation(x, P, z, R)
        d.append(T.distance2(y, Si))
    assert d[0] == d[1] and d[0] <= 16.27
    assert (dets[0].state, dets[0].id) == (T.DET_MATCHED, 1) and (dets[1].state, dets[1].id) == (T.DET_STARTED, 2)


def test_ineligible_observations_get_state_0_and_never_match(ref):
    sc, res = ref["ineligible"]
    for (t, _, _, obs), (dets, frame, _) in zip(sc["frames"], res):
        good = [i for i, o in enumerate(obs) if o.valid == 1 and o.cov is None and all(map(math.isfinite, o.tvec)) and 0 < o.tvec[2] < 1e100]
        assert len(good) == 1
        for i, d in enumerate(dets):
            if i in good:
                assert d.state in (T.DET_MATCHED, T.DET_STARTED) and d.id == 1
            else:
                assert T.pack_det_track(d) == bytes(T.DET_TRACK_SIZE)
        assert frame.n_live == 1


def test_a_stamp_that_does_not_rise_is_refused_and_leaves_the_table_alone(ref):
    sc, _ = ref["stale"]
    tr = T.Tracker(sc["opts"])
    states = []
    for t, Rw, tw, obs in sc["frames"]:
        before = b"".join(T.pack_track(x) for x in tr.snapshot()), tr.stamp, tr.next_id
        dets, frame, snap = tr.update(t, obs, Rw, tw)
        states.append(frame.state)
        if frame.state == T.FRAME_STALE:
            assert (b"".join(T.pack_track(x) for x in tr.snapshot()), tr.stamp, tr.next_id) == before
            assert b"".join(T.pack_track(x) for x in snap) == before[0]
            assert all(T.pack_det_track(d) == bytes(T.DET_TRACK_SIZE) for d in dets) and len(dets) == len(obs)
    assert states == [1, 1, 1, -2, -2, -2, 1, 1]
    assert tr.tracks[0].hits == 5 and tr.tracks[0].state == T.CONFIRMED


def test_P_stays_exactly_symmetric_with_a_positive_diagonal_through_1000_frames(ref):
    _, res = ref["long_1000"]
    assert len(res) == 1000
    for _, frame, snap in res:
        assert frame.state == 1 and frame.n_live >= 2   # (a 0.999 gate misses now and then: a third track may live for a while)
        for tr in [t for t in snap if t.state != T.FREE]:
            assert all(tr.P[i][j] == tr.P[j][i] for i in range(6) for j in range(i))
            assert all(tr.P[i][i] > 0.0 for i in range(6))
    assert sum(len(d) for d, _, _ in res) == 2000 and res[-1][1].n_confirmed >= 2


def test_a_static_point_seen_from_a_moving_camera_gets_zero_velocity(ref):
    _, res = ref["static_point"]
    tr = res[-1][2][0]
    assert tr.id == 1 and tr.hits == len(res)
    speed = math.sqrt(sum(v * v for v in tr.x[3:]))
    early = math.sqrt(sum(v * v for v in res[5][2][0].x[3:]))
    print("speed after 6 frames:", early, "after 300:", speed)
    assert speed < 0.25 and max(abs(tr.x[0] - 0.5), abs(tr.x[1] + 0.2), abs(tr.x[2] - 5.0)) < 0.05
    mean = [sum(r[2][0].x[3 + a] for r in res[100:]) / 200 for a in range(3)]
    assert max(abs(m) for m in mean) < 0.1


# ---- host-side ABI ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def test_struct_sizes_match_the_header_and_the_packers(tmp_path, lib):
    src = tmp_path / "tk.c"
    names = ["irmv_track_opts", "irmv_det_track", "irmv_track_frame", "irmv_track", "irmv_track_obs"]
    src.write_text('#include <stdio.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(f'printf("%zu ", sizeof({n}));' for n in names) + "return 0;}\n")
    exe = tmp_path / "tk"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [72, T.DET_TRACK_SIZE, T.FRAME_SIZE, T.TRACK_SIZE, 112]
    assert got == [C.sizeof(c) for c in (capi.TrackOpts, capi.DetTrack, capi.TrackFrame, capi.Track, capi.TrackObs)]
    lim = (C.c_int32 * 8)()
    assert lib.irmv_track_limits(lim) == 0
    assert list(lim) == [32, 384, 72, 40, 72, 256, 0, 0]


def test_the_library_defaults_are_the_reference_defaults(lib):
    """irmv_track_default_opts is where the facades take the defaults from; tracks.Options states them for the reference."""
    o = capi.TrackOpts()
    assert lib.irmv_track_default_opts(C.byref(o)) == 0 and lib.irmv_track_default_opts(None) == capi.ERR_ARG
    want = T.Options()
    assert (o.struct_size, o.enable, o.reserved) == (72, 0, 0)
    for name in ("confirm_hits", "max_misses", "match_class", "gate", "max_coast_s", "accel_sigma", "init_vel_sigma", "sigma_lat", "sigma_rng"):
        assert getattr(o, name) == getattr(want, name), name
    assert bytes(capi.track_opts_struct(0)) == bytes(o) and capi.track_opts_struct(gate=9.0).gate == 9.0
    with pytest.raises(TypeError):
        capi.track_opts_struct(gait=9.0)


def test_option_values_are_refused_on_the_host_values_first(lib):
    """A refused value never reaches an engine: the call fails with IRMV_ERR_ARG on a NULL engine for the value's sake."""
    nan, inf = float("nan"), float("inf")
    for field in ("gate", "max_coast_s", "accel_sigma", "init_vel_sigma", "sigma_lat", "sigma_rng"):
        for bad in (0.0, -1.0, nan, inf, -inf):
            o = capi.track_opts_struct(**{field: bad})
            assert lib.irmv_engine_set_tracking(None, C.byref(o)) == capi.ERR_ARG
            assert b"finite and positive" in lib.irmv_last_error(), (field, bad)
            with pytest.raises(ValueError):
                T.check_options(T.Options(**{field: bad}))
    for field, bad in (("enable", 2), ("match_class", -1), ("confirm_hits", 0), ("max_misses", 0), ("confirm_hits", (1 << 20) + 1)):
        o = capi.track_opts_struct(**{field: bad})
        assert lib.irmv_engine_set_tracking(None, C.byref(o)) == capi.ERR_ARG
        assert field.encode() in lib.irmv_last_error()
        with pytest.raises(ValueError):
            T.check_options(T.Options(**{field: bad}))
    o = capi.track_opts_struct()
    o.struct_size = 8
    assert lib.irmv_engine_set_tracking(None, C.byref(o)) == capi.ERR_ARG and b"struct_size" in lib.irmv_last_error()
    o = capi.track_opts_struct()
    o.reserved = 1
    assert lib.irmv_engine_set_tracking(None, C.byref(o)) == capi.ERR_ARG and b"reserved" in lib.irmv_last_error()
    assert lib.irmv_engine_set_tracking(None, None) == capi.ERR_ARG
    assert lib.irmv_engine_set_tracking(None, C.byref(capi.track_opts_struct())) == capi.ERR_ARG and b"engine is null" in lib.irmv_last_error()
    assert lib.irmv_engine_set_stamp(None, 0, nan) == capi.ERR_ARG and b"finite" in lib.irmv_last_error()


def test_track_predict_has_the_reference_bits(ref, lib):
    _, res = ref["three_200"]
    checked = 0
    for f in (0, 3, 57, 199):
        for tr in res[f][2][:3]:
            c = capi.Track.from_buffer_copy(T.pack_track(tr))
            for dt in (0.0, 0.004, 0.05, 1.7):
                pos, cov = (C.c_double * 3)(), (C.c_double * 9)()
                assert lib.irmv_track_predict(C.byref(c), tr.stamp + dt, 8.0, pos, cov) == 0
                epos, ecov = T.predict_position(tr, tr.stamp + dt, 8.0)
                assert struct.pack("<3d", *pos) == struct.pack("<3d", *epos) and struct.pack("<9d", *cov) == struct.pack("<9d", *ecov)
                checked += 1
    assert checked == 48
    c = capi.Track.from_buffer_copy(T.pack_track(res[10][2][0]))
    pos, cov = (C.c_double * 3)(), (C.c_double * 9)()
    assert lib.irmv_track_predict(C.byref(c), c.stamp - 0.01, 8.0, pos, cov) == capi.ERR_ARG
    assert lib.irmv_track_predict(C.byref(c), c.stamp + 0.01, 0.0, pos, cov) == capi.ERR_ARG
    assert lib.irmv_track_predict(C.byref(c), float("nan"), 8.0, pos, cov) == capi.ERR_ARG
    free = capi.Track()
    assert lib.irmv_track_predict(C.byref(free), 1.0, 8.0, pos, cov) == capi.ERR_ARG
    assert lib.irmv_track_predict(None, 1.0, 8.0, pos, cov) == capi.ERR_ARG
