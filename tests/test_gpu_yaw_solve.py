"""The constrained pose on the GPU (include/irmv_hip.h, "constrained pose"; csrc/k_yaw.hip): irmv_pnp_solve_yaw and the step's
side records against irmv_detection_amd.yaw_solve, the host reference that follows the kernel operation for operation.

Smallest shapes: a 128 x 64 net on a 1280 x 1024 source, heads injected with write_head + run_post (tests/pose_prior_set.py
quad_head: 32 quads a frame), as tests/test_gpu_pose_prior.py does.  The reference is always fed the keypoints a step
REPORTS, the float32 the kernel saw, and the unit up vector the engine holds.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import pnp_ref as P
import pose_prior_set as L
import refine_craft as rc
import yaw_set as YS
from irmv_detection_amd import capi, pose_prior as pp, yaw_solve as Y
from irmv_detection_amd.engine import PnPSolver, YoloEngine

pytestmark = pytest.mark.gpu

SRC, NET = (1280, 1024), (128, 64)
K, D, CAM = YS.K, YS.D, YS.CAM
PER = 32


def eng(blob, **kw):
    kw.setdefault("camera_matrix", K)
    kw.setdefault("dist_coeffs", list(D))
    return YoloEngine(None, kw.pop("src", SRC), weights_blob=blob, net_size=NET[0], net_height=NET[1], armor_size=L.SIZE, **kw)


def run(e, quads, slot=0, src=SRC, classes=None):
    head, _ = L.quad_head(e, src, quads, classes)
    e.write_head(head, slot)
    e.run_post(slot, 1)
    d = e.results_raw(slot)
    assert len(d) == len(quads)
    return d


def kpts_of(d):
    return np.array(list(d.kpts), np.float32)


def rot_of(y):
    return _quat_matrix(np.array(list(y.quat)))


def _quat_matrix(q):
    x, y, z, w = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def by_up(cases):
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault(c["u"].tobytes(), []).append(i)
    return [(np.frombuffer(k, np.float64), v) for k, v in groups.items()]


def check_record(y, pts, u, s, where, rounds=4, tau_max=1.0, size=L.SIZE):
    """One solved device record against the reference: tau within one final-round step of the reference's own; the reference
    evaluated AT the device's tau gives its R (from quat), tvec and err to 1e-12 relative and its rvec to 1e-9.
    -> (lanes equal, bits equal)."""
    ref = Y.solve(CAM, pts, size, u, s, rounds=rounds, tau_max=tau_max)
    assert y.state == 1 and ref["state"] == 1, (where, y.state, ref["state"])
    assert abs(y.tau - ref["tau"]) <= ref["step"], (where, y.tau, ref["tau"], ref["step"])
    at = Y.at_tau(CAM, pts, size, u, s, y.tau)
    t = np.array(list(y.tvec))
    assert np.abs(rot_of(y) - at["R"]).max() <= 1e-12, (where, np.abs(rot_of(y) - at["R"]).max())
    assert np.abs(t - at["t"]).max() <= 1e-12 * np.abs(at["t"]).max(), (where, t, at["t"])
    assert abs(y.err - at["err"]) <= 1e-12 * at["err"], (where, y.err, at["err"])
    assert abs(y.cs - float(at["cs"])) <= 1e-15 and abs(y.sn - float(at["sn"])) <= 1e-15, where
    assert np.abs(np.array(list(y.rvec)) - P.rvec_of(at["R"])).max() <= 1e-9, where
    lanes = list(y.lane) == ref["lane"]
    bits = lanes and np.array([y.tau, y.err] + list(y.tvec)).tobytes() == np.array([ref["tau"], ref["err"]] + list(ref["t"])).tobytes()
    return lanes, bits


# ---- 1. irmv_pnp_solve_yaw over the lean-back set ----------------------------------------------------------------------
def test_solve_yaw_over_the_lean_back_set(capsys):
    """All 400 quads in one call, once per up vector of the set (the call takes one for all its quads): every case is
    checked in the call that carries its own up vector, none is left out."""
    cases = L.lean_back_set()
    pts = np.stack([c["pts"].reshape(8) for c in cases])
    s = PnPSolver(K, list(D))
    seen = dict(n=0, lanes=0, bits=0)
    try:
        for u, idx in by_up(cases):
            out = s.solve_yaw(pts, u, L.S, L.SIZE)
            assert len(out) == len(cases)
            un = pp.normalise_up(u)
            for i in idx:
                lanes, bits = check_record(out[i], cases[i]["pts"], un, L.S, i)
                seen["n"] += 1; seen["lanes"] += lanes; seen["bits"] += bits
        # refusals of the stand-alone form
        assert all(y.state == -1 and list(y.lane) == [-1] * 6 and y.tau == 0.0 for y in s.solve_yaw(pts[:5], (0.0, 0.0, 1.0), L.S))
        assert all(y.state == -1 for y in s.solve_yaw(pts[:5], cases[0]["u"], 1.0))
        bad = pts[:3].copy(); bad[1, 3] = np.nan
        st = [y.state for y in s.solve_yaw(bad, cases[0]["u"], L.S)]
        assert st[1] == 0 and st[0] != 0 and st[2] != 0
        one = s.solve_yaw(pts[:1], cases[0]["u"], L.S, rounds=2)[0]
        assert list(one.lane)[2:] == [-1] * 4 and one.lane[0] >= 0
    finally:
        s.close()
    with capsys.disabled():
        print(f"\n[yaw solve] irmv_pnp_solve_yaw over the lean-back set: {seen}")
    assert seen["n"] == len(cases)


# ---- 2. through an engine, beside the prior (fails on a build without the feature: the calls do not exist) ------------------
def test_engine_records_on_the_cases_the_prior_gets_wrong(blob, capsys):
    cases = L.lean_back_set()
    stats = dict(n=0, hard=0, dev_bad=0, ref_bad=0, lanes=0)
    with eng(blob) as e:
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
        e.set_yaw_solve()
        assert e.yaw_solve() == dict(enable=True, rounds=4, tau_max=1.0, horizon_min=1e-4)
        for u, idx in by_up(cases):
            e.set_up(u)
            un = e.up()
            for k in range(0, len(idx), PER):
                part = [cases[i] for i in idx[k:k + PER]]
                dets = run(e, [c["pts"] for c in part])
                yaws = e.yaw_poses(0)
                assert len(yaws) == len(dets)
                for c, d, y in zip(part, dets, yaws):
                    stats["n"] += 1
                    assert d.pnp_ok == 1 and y.state == 1
                    if Y.yaw_error(P.matrix_of(np.array(list(d.rvec))), c["R"], c["u"]) <= 10.0:
                        continue
                    ref = Y.solve(CAM, kpts_of(d), L.SIZE, un, L.S)
                    assert ref["state"] == 1 and abs(y.tau - ref["tau"]) <= ref["step"]
                    stats["hard"] += 1
                    stats["lanes"] += list(y.lane) == ref["lane"]
                    stats["dev_bad"] += Y.yaw_error(rot_of(y), c["R"], c["u"]) > 10.0
                    stats["ref_bad"] += Y.yaw_error(ref["R"], c["R"], c["u"]) > 10.0
    with capsys.disabled():
        print(f"\n[yaw solve] engine, mode PRIOR, lean-back set: {stats}")
    assert stats["n"] == len(cases) and stats["hard"] >= 30
    assert stats["dev_bad"] == stats["ref_bad"] < stats["hard"]


# ---- 3. irmv_det and irmv_pose_alt do not notice ---------------------------------------------------------------------------
def _snapshot(e):
    return [bytes(d) for d in e.results_raw(0)], [bytes(a) for a in e.pose_alts(0)]


def test_records_are_untouched_keypoint(blob):
    Z = P.zoo()
    frames = [[Z[i]["pts"] for i in range(k * PER, (k + 1) * PER)] for k in range(2)] + [[c["pts"] for c in L.lean_back_set()[:PER]]]
    with eng(blob) as never, eng(blob) as e:
        for x in (never, e):
            x.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
            x.set_up((0.1, -1.0, 0.2))
        want = []
        for q in frames:
            run(never, q)
            want.append(_snapshot(never))
        n = C.c_int(0)
        assert e._L.irmv_engine_yaw_poses(e._h, 0, (capi.YawPose * e.max_det)(), e.max_det, C.byref(n)) == capi.ERR_ARG
        e.set_yaw_solve()
        solved = 0
        for q, w in zip(frames, want):
            dets = run(e, q)
            assert _snapshot(e) == w
            ys = e.yaw_poses(0)
            assert all((y.state != 0) == bool(d.pnp_ok) for d, y in zip(dets, ys))
            solved += sum(y.state == 1 for y in ys)
        assert solved >= PER
        e.set_yaw_solve(enable=False)
        for q, w in zip(frames, want):
            run(e, q)
            assert _snapshot(e) == w
            assert all(bytes(y) == bytes(capi.YawPose()) for y in e.yaw_poses(0))
        # enabled -> disabled -> enabled with no step in between: nothing of the last enabled step is shown
        run(e, frames[2])
        e.set_yaw_solve()
        run(e, frames[2])
        assert sum(y.state == 1 for y in e.yaw_poses(0)) >= PER // 2
        e.set_yaw_solve(enable=False)
        e.set_yaw_solve()
        assert len(e.yaw_poses(0)) == PER and all(bytes(y) == bytes(capi.YawPose()) for y in e.yaw_poses(0))
        run(e, frames[2])
        assert sum(y.state == 1 for y in e.yaw_poses(0)) >= PER // 2


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_records_are_untouched_classical_and_refined(blob, source):
    """The eight-plate scene of the refined tests as a whole step (detect(): the op stands behind the light extraction)."""
    sblob = rc.step_blob(blob)
    img, _ = rc.step_scene()
    mk = lambda: YoloEngine(None, rc.SRC, weights_blob=sblob, net_size=rc.NET[0], net_height=rc.NET[1], point_source=source)   # noqa: E731
    with mk() as never, mk() as e:
        for x in (never, e):
            x.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
            x.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        never.detect()
        want = _snapshot(never)
        assert len(want[0]) >= 4
        e.set_yaw_solve()
        e.detect()
        assert _snapshot(e) == want
        dets, ys = e.results_raw(0), e.yaw_poses(0)
        for d, y in zip(dets, ys):
            assert (y.state != 0) == (d.pnp_ok == 1 and d.armor_valid == 1)
            if y.state == 1:      # the record is the constrained pose of the quad irmv_det finally reports
                check_record(y, kpts_of(d), e.up(), L.S, "step")
        # (the classical pairing finds no armor in this scene's boxes: its solved records are
        # test_classical_engine_solves_drawn_plates')
        assert source == capi.POINTS_CLASSICAL or sum(y.state == 1 for y in ys) >= 4
        e.set_yaw_solve(enable=False)
        e.detect()
        assert _snapshot(e) == want


def test_classical_engine_solves_drawn_plates(blob):
    """OP_YAW behind OP_LIGHT on records the light extraction solved: zoo poses drawn as two bright bars with one box around
    them (the recipe of tests/test_gpu_pose_prior.py test_scalar_form_alts_equal_solve2), run_post on a classical engine.  The
    record is the reference's on the four points the extraction reports; at least two are solved (state 1)."""
    from oracle import oracle
    from test_gpu_pnp import _draw_bar
    from test_gpu_pose_prior import _box_head
    done = solved = 0
    with eng(blob, rotate180=False, point_source=capi.POINTS_CLASSICAL) as e:
        e.set_yaw_solve()
        for c in P.zoo():
            if done >= 6:
                break
            q = c["pts"].astype(np.float64)
            if c["cam"] != L.CAM or c["size"] != L.SIZE or c["R"] is None or q[:, 0].min() < 60 or q[:, 0].max() > 1220 or q[:, 1].min() < 60 or q[:, 1].max() > 964:
                continue
            ll, lr = np.linalg.norm(q[1] - q[0]), np.linalg.norm(q[3] - q[2])
            if min(ll, lr) < 14 or max(ll, lr) > 300:
                continue
            img = np.zeros((SRC[1], SRC[0], 3), np.uint8)
            _draw_bar(img, q[0], q[1], 0.2 * ll)
            _draw_bar(img, q[3], q[2], 0.2 * lr)
            e.get_src_image_buffer()[:] = img
            e.detect()                                     # the frame into the slot's device frame
            e.write_head(_box_head(e, SRC, q), 0)
            e.run_post(0, 1)
            dets, ys = e.results_raw(0), e.yaw_poses(0)
            assert len(dets) == 1 and len(ys) == 1
            if not oracle.extract_armor(img, np.array(dets[0].xyxy, np.float32))["ok"] or not dets[0].pnp_ok:
                continue
            assert dets[0].armor_valid == 1
            ref = Y.solve(CAM, kpts_of(dets[0]), dets[0].armor_size, e.up(), L.S)
            assert ys[0].state == ref["state"] != 0, (c["name"], ys[0].state, ref["state"])
            if ys[0].state == 1:
                check_record(ys[0], kpts_of(dets[0]), e.up(), L.S, c["name"], size=dets[0].armor_size)
                solved += 1
            done += 1
    assert done >= 4 and solved >= 2


# ---- 4. live setters -----------------------------------------------------------------------------------------------------------
def test_two_slots_with_their_own_up_and_live_setters(blob):
    """One batched run_post of two slots with the same head and different up vectors; set_up, set_pose_prior and a second
    set_yaw_solve capture nothing anew and take effect in the next step."""
    groups = by_up(L.lean_back_set())
    (u0, idx0), (u1, _) = groups[0], groups[1]
    part = [L.lean_back_set()[i] for i in idx0[:PER]]
    quads = [c["pts"] for c in part]

    def check(e, ups, s, rounds=4, tau_max=1.0):
        taus = []
        for slot, uu in enumerate(ups):
            un = e.up(slot)
            assert np.array_equal(un, pp.normalise_up(uu))
            dets, ys = e.results_raw(slot), e.yaw_poses(slot)
            assert len(ys) == len(quads)
            for j, (d, y) in enumerate(zip(dets, ys)):
                check_record(y, kpts_of(d), un, s, (slot, j), rounds, tau_max)
            taus.append([y.tau for y in ys])
        return taus

    with eng(blob, num_slots=2) as e:
        head, _ = L.quad_head(e, SRC, quads)
        e.set_yaw_solve()
        e.set_pose_prior("min_err", 8.0, L.S)
        e.set_up(u0, 0)
        e.set_up(u1, 1)
        for s in (0, 1):
            e.write_head(head, s)
        e.run_post(0, 2)
        g0 = e.debug_graph_count()
        t = check(e, (u0, u1), L.S)
        assert max(abs(a - b) for a, b in zip(*t)) > 1e-3          # the two slots did solve with their own vectors
        e.set_up(u1, 0)
        e.set_up(u0, 1)
        e.run_post(0, 2)
        assert e.debug_graph_count() == g0
        assert check(e, (u1, u0), L.S) == [t[1], t[0]]
        e.set_pose_prior("min_err", 8.0, 0.1)                      # another tilt
        e.set_yaw_solve(rounds=2, tau_max=2.0)
        e.run_post(0, 2)
        assert e.debug_graph_count() == g0
        check(e, (u1, u0), 0.1, 2, 2.0)
        assert all(list(y.lane)[2:] == [-1] * 4 for y in e.yaw_poses(0))
        with pytest.raises(capi.IrmvError):
            e.set_yaw_solve(rounds=7)
        assert e.yaw_solve()["rounds"] == 2


def test_window_move_and_frame_view_keep_the_records(blob):
    """A window engine: the same full-frame quads before and after a window move, and in the frame view.  The crop only moves
    the principal point and u is untouched, so the records agree up to what the keypoints' float32 rounding does: <= 5e-4 px
    (tests/test_gpu_pose_prior.py states the bound), and 0.5 px of noise moves tau by < 0.1 and the pose by < 1 (rad, m) on
    this set: 1e-3 is generous."""
    FULL, WIN = (322, 201), (256, 128)
    groups = by_up(L.lean_back_set())
    u, idx = groups[0]
    quads = [L.lean_back_set()[i]["pts"].astype(np.float64) for i in idx[:24]]
    snaps = []
    with YoloEngine(None, FULL, weights_blob=blob, net_size=NET[0], net_height=NET[1], window=WIN, camera_matrix=K, dist_coeffs=list(D),
                    armor_size=L.SIZE, rotate180=False) as e:
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
        e.set_up(u)
        e.set_yaw_solve()
        for view, org in (("window", (0, 0)), ("window", (66, 73)), ("window", (13, 40)), ("frame", (0, 0))):
            e.set_view(view)
            if view == "window":
                e.set_window(*org)
            dets = run(e, [q - np.array(org, np.float64) for q in quads], src=WIN if view == "window" else FULL)
            ys = e.yaw_poses(0)
            assert all(d.pnp_ok for d in dets) and all(y.state == 1 for y in ys)
            snaps.append(np.stack([[y.tau] + list(y.rvec) + list(y.tvec) for y in ys]))
    for s in snaps[1:]:
        assert np.abs(s - snaps[0]).max() <= 1e-3


def test_tiled_step_records_by_tile_and_index(blob):
    """One tiled step of two windows: each slot's records are, byte for byte, those of the ordinary step on the same window,
    and the record of merged record r is yaw_poses(first + r.tile)[r.index]."""
    from test_gpu_window import FULL, WIN, frame_of
    wblob = dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))
    corners = [(0, 0), (66, 73)]
    frame = frame_of(12)
    with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, num_slots=3, camera_matrix=K) as e:
        e.set_yaw_solve()
        for s in range(3):
            e.set_up((0.1, -1.0, 0.2), s)
            e.get_src_image_buffer(s)[:] = frame
        e.set_tiles(corners, 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        recs, _ = e.tile_results_raw(1)
        tiled = [([bytes(d) for d in e.results_raw(1 + t)], [bytes(y) for y in e.yaw_poses(1 + t)]) for t in range(2)]
        ys = [e.yaw_poses(1 + t) for t in range(2)]
        assert len(recs) >= 1
        solved = 0
        for r in recs:
            assert bytes(r.det) == tiled[r.tile][0][r.index]
            y = ys[r.tile][r.index]
            assert (y.state != 0) == bool(r.det.pnp_ok)
            solved += y.state == 1
        assert solved >= 1
        for t in range(2):
            e.submit(1 + t, 1)
            e.wait_slots(1 + t, 1)
            assert [bytes(d) for d in e.results_raw(1 + t)] == tiled[t][0]
            assert [bytes(y) for y in e.yaw_poses(1 + t)] == tiled[t][1]


# ---- 5. refused records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, 1e8], ids=["nan", "2^24"])
def test_bad_keypoint_empties_one_record_only(blob, bad):
    u, idx = by_up(L.lean_back_set())[0]
    quads = [L.lean_back_set()[i]["pts"] for i in idx[:12]]
    with eng(blob) as e:
        e.set_up(u)
        e.set_yaw_solve()
        head, anchors = L.quad_head(e, SRC, quads)
        nc = e.head_channels - 64 - 8
        e.write_head(head, 0); e.run_post(0, 1)
        clean = [bytes(y) for y in e.yaw_poses(0)]
        assert all(y.state == 1 for y in e.yaw_poses(0))
        for hit, k in ((3, 0), (8, 5)):
            dirty = head.copy()
            dirty[anchors[hit], 64 + nc + k] = bad
            e.write_head(dirty, 0); e.run_post(0, 1)
            d, ys = e.results_raw(0), e.yaw_poses(0)
            assert len(ys) == len(quads) and d[hit].pnp_ok == 0 and ys[hit].state == 0 and bytes(ys[hit]) == bytes(capi.YawPose())
            assert all(bytes(ys[j]) == clean[j] for j in range(len(quads)) if j != hit)


def test_no_basis_refuses(blob):
    """u along the optical axis: every record of the slot is refused; a class with |s| = 1: that class's records are."""
    u, idx = by_up(L.lean_back_set())[0]
    quads = [L.lean_back_set()[i]["pts"] for i in idx[:12]]
    with eng(blob) as e:
        e.set_yaw_solve()
        e.set_up((0.0, 0.0, 1.0))
        dets = run(e, quads)
        ys = e.yaw_poses(0)
        assert all(d.pnp_ok for d in dets)
        assert all(y.state == -1 and list(y.lane) == [-1] * 6 and y.tau == 0.0 and y.err == 0.0 for y in ys)
        e.set_up(u)
        nu = np.full(16, L.S)
        nu[3], nu[5] = 1.0, -1.0
        e.set_pose_prior("min_err", 8.0, nu)
        dets = run(e, quads)
        ys = e.yaw_poses(0)
        assert sorted({d.class_id for d in dets} & {3, 5}) == [3, 5]
        for d, y in zip(dets, ys):
            assert y.state == (-1 if d.class_id in (3, 5) else 1), (d.class_id, y.state)


# ---- 6. memory residue ---------------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_what_device_memory_held(blob):
    u, idx = by_up(L.lean_back_set())[0]
    quads = [L.lean_back_set()[i]["pts"] for i in idx[:PER]]

    def go(fill):
        with eng(blob) as e:
            e.set_up(u)
            e.set_yaw_solve()
            names = {r["name"]: r["cls"] for r in e.debug_allocs()}
            assert names["yaw_dev"] == "SCRATCH" and names["yaw_table"] == "CONST" and names["yaw_basis"] == "CONST"
            if fill is not None:
                assert e.debug_fill_mem(fill) > 0
            run(e, quads)
            return [bytes(d) for d in e.results_raw(0)], [bytes(y) for y in e.yaw_poses(0)]

    fresh = go(None)
    assert all(capi.YawPose.from_buffer_copy(b).state == 1 for b in fresh[1])
    for pattern in (0xFFFFFFFF, 0x7C007C00):
        assert go(pattern) == fresh
