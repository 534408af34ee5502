"""The pose uncertainty on the GPU (include/irmv_hip.h, "pose uncertainty"; csrc/k_posecov.hip): irmv_pnp_pose_cov and the
step's side records against irmv_detection_amd.pose_cov, the host reference that follows the kernel operation for operation
-- BIT FOR BIT, every field.

Smallest shapes: a 128 x 64 net on a 256 x 128 source (the window tests' sizes), whole steps on the crafted Detect finals of
tests/test_gpu_window.py (class logits shifted up, an armor-like quad around each anchor).  The reference is always fed the
keypoints, the pose and the constrained pose a step REPORTS, and the unit up vector the engine holds.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import mem_residue as MR
import pnp_ref as P
import pose_cov_set as S
import refine_craft as rc
import test_gpu_numbers as TN
from irmv_detection_amd import capi, frames, pose_cov as pc, window, yaw_solve as ys
from irmv_detection_amd.engine import DEFAULT_CAMERA_MATRIX, DEFAULT_DIST_COEFFS, PnPSolver, YoloEngine
from test_gpu_window import FULL, K, NET, WIN, frame_of

pytestmark = pytest.mark.gpu

CAM = ys.camera_of(K, DEFAULT_DIST_COEFFS)
SIGMA = 0.7
ZERO = bytes(capi.PoseCov())


@pytest.fixture(scope="module")
def wblob(blob):
    return dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))


@pytest.fixture(scope="module")
def solver():
    s = PnPSolver(K, list(DEFAULT_DIST_COEFFS))
    yield s
    s.close()


def peng(blob, src=WIN, **kw):
    kw.setdefault("camera_matrix", K)
    return YoloEngine(None, src, weights_blob=blob, net_size=NET[0], net_height=NET[1], **kw)


def put(e, frame, slot=0):
    e.get_src_image_buffer(slot)[:] = frame


def win_frame(i):
    return frames.synthetic_frame(i, WIN[0], WIN[1])


def covs_bytes(e, slot=0):
    return [bytes(c) for c in e.pose_covs(slot)]


def check_slot(e, slot, sigma, cam=CAM, solver=None):
    """The slot's records against the reference on the step's own irmv_det / irmv_yaw_pose records (and, with a solver,
    against irmv_pnp_pose_cov on them) -> (records with state 1, records with yaw_state 1)."""
    dets, covs = e.results_raw(slot), e.pose_covs(slot)
    yaw_on = e.yaw_solve()["enable"]
    yaws = e.yaw_poses(slot) if yaw_on else [None] * len(dets)
    assert len(covs) == len(dets)
    u = tuple(float(v) for v in e.up(slot))
    n1 = ny = 0
    for j, (d, c, y) in enumerate(zip(dets, covs, yaws)):
        if not (d.pnp_ok == 1 and d.armor_valid == 1):
            assert bytes(c) == ZERO, (slot, j)
            continue
        kp = np.array(list(d.kpts), np.float32)
        yaw = (list(y.rvec), list(y.tvec), u) if (y is not None and y.state == 1) else None
        ref = pc.pose_cov(cam, kp, d.armor_size, list(d.rvec), list(d.tvec), sigma, yaw=yaw)
        assert S.same_bits(c, ref), (slot, j, S.first_difference(c, ref))
        n1 += c.state == 1
        ny += c.yaw_state == 1
        if solver is not None:
            a = solver.pose_cov(kp, list(d.rvec), list(d.tvec), d.armor_size, sigma_px=sigma)[0]
            assert bytes(a)[:23 * 8] == bytes(c)[:23 * 8] and a.state == c.state and a.yaw_state == 0, (slot, j)
            if yaw is not None and pc.unit(u) == u:      # (the call normalises its up vector again)
                b = solver.pose_cov(kp, list(y.rvec), list(y.tvec), d.armor_size, up=u, sigma_px=sigma)[0]
                assert bytes(b)[23 * 8:] == bytes(c)[23 * 8:], (slot, j)
    return n1, ny


# ---- 1. irmv_pnp_pose_cov -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 65, 256])
def test_pnp_pose_cov_on_the_hard_set(n):
    """The CPU test's hard set, per camera and plate size, cycled to n quads, with and without an up vector."""
    seen = 0
    for cam in (0, 2):
        _, Kc, Dc = P.CAMERAS[cam]
        s = PnPSolver(Kc, list(Dc))
        try:
            for size in (0, 1):
                sub = [c for c in S.hard_set() if c["cam"] == cam and c["size"] == size]
                pick = [sub[i % len(sub)] for i in range(n)]
                for up in (None, sub[0]["u"]):
                    out = s.pose_cov(np.array([c["pts"] for c in pick]).reshape(-1, 8), np.array([c["rvec"] for c in pick]).reshape(-1, 3),
                                     np.array([c["t"] for c in pick]).reshape(-1, 3), size, up=up, sigma_px=SIGMA)
                    assert len(out) == n
                    for c, o in zip(pick, out):
                        ref = _hard_reference(c["name"], None if up is None else tuple(up))
                        assert S.same_bits(o, ref), (c["name"], up is None, S.first_difference(o, ref))
                        assert o.state == 1 and o.yaw_state == (0 if up is None else 1)
                        seen += 1
        finally:
            s.close()
    assert seen == 8 * n


_hard = {}


def _hard_reference(name, up):
    if (name, up) not in _hard:
        c = next(c for c in S.hard_set() if c["name"] == name)
        _hard[(name, up)] = S.reference(dict(c, u=up or c["u"]), SIGMA, up is not None)
    return _hard[(name, up)]


def test_pnp_pose_cov_refusals(solver):
    """Each refusal rule on the device: state -1 and everything else zero, the neighbours untouched."""
    q = np.array([300.0, 330, 300, 270, 420, 270, 420, 330], np.float32)
    r0, t0 = (0.0, 0.0, 0.0), (0.0, 0.0, 2.0)
    good = solver.pose_cov(q, r0, t0)[0]
    assert S.same_bits(good, pc.pose_cov(CAM, q, 0, r0, t0)) and good.state == 1
    bad_q = q.copy(); bad_q[5] = np.nan
    big_q = q.copy(); big_q[0] = 2.0 ** 24
    cases = [(bad_q, r0, t0), (big_q, r0, t0), (q, r0, (0.0, 0.0, 0.01)), (q, r0, (0.0, 0.0, -2.0)), (q, r0, (0.0, 0.0, 1e160)),
             (q, (np.nan, 0.0, 0.0), t0), (q, r0, (np.inf, 0.0, 2.0))]
    pts = np.array([q] + [c[0] for c in cases] + [q])
    rv = np.array([r0] + [c[1] for c in cases] + [r0])
    tv = np.array([t0] + [c[2] for c in cases] + [t0])
    out = solver.pose_cov(pts, rv, tv)
    assert bytes(out[0]) == bytes(good) == bytes(out[-1])
    for o, c in zip(out[1:-1], cases):
        assert S.is_zero_record(o, -1) and S.same_bits(o, pc.pose_cov(CAM, *c[:1], 0, c[1], c[2]))
    # the yaw block refuses alone
    o = solver.pose_cov(q, r0, t0, up=(0.0, -1.0, 0.0))[0]
    assert o.state == 1 and o.yaw_state == 1
    with pytest.raises(capi.IrmvError):
        solver.pose_cov(q, r0, t0, sigma_px=0.0)


# ---- 2. in the step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [False, True], ids=["yaw-off", "yaw-on"])
def test_step_records_equal_the_reference(wblob, solver, yaw):
    """detect() at counts max_det = 100-or-fewer, max_det = 5, 1 and 0 (a blob whose class logits stay dark)."""
    dark = dc.craft(wblob, cls=("shift", -60.0))
    for blob_, max_det, want in ((wblob, 100, None), (wblob, 5, 5), (wblob, 1, 1), (dark, 100, 0)):
        with peng(blob_, max_det=max_det) as e:
            n = C.c_int(0)
            assert e._L.irmv_engine_pose_covs(e._h, 0, (capi.PoseCov * e.max_det)(), e.max_det, C.byref(n)) == capi.ERR_ARG
            assert e.pose_cov() == dict(enable=False, sigma_px=1.0)
            if yaw:
                e.set_yaw_solve()
            e.set_pose_cov(sigma_px=SIGMA)
            assert e.pose_cov() == dict(enable=True, sigma_px=SIGMA)
            put(e, win_frame(12))
            e.detect()
            dets = e.results_raw(0)
            assert want is None or len(dets) == want, (max_det, len(dets))
            n1, ny = check_slot(e, 0, SIGMA, solver=solver)
            if want == 0:
                assert e.pose_covs(0) == []
            else:
                assert n1 >= 1 and (ny >= 1) == yaw and (yaw or all(c.yaw_state == 0 and not any(c.yaw_cov) for c in e.pose_covs(0)))


# ---- 3. every launch form -------------------------------------------------------------------------------------------------------
def test_graph_and_eager_and_batched_submits(wblob, monkeypatch):
    """detect() launched as a graph and kernel by kernel; a batched submit of 2 and of 5 slots on two streams with a frame
    (and so a count) of its own per slot, slot 1 with an up vector of its own: each slot's records are the reference's, and the
    bytes of a one-slot engine's detect() on the same frame."""
    fr = [win_frame(20 + i) for i in range(5)]
    single = {}
    for mode in ("graph", "eager"):
        monkeypatch.setenv("IRMV_SYNC_LAUNCH", mode)
        with peng(wblob) as e:
            assert e.sync_launch == mode
            e.set_yaw_solve()
            e.set_pose_cov(sigma_px=SIGMA)
            got = []
            for f in fr:
                put(e, f)
                e.detect()
                assert check_slot(e, 0, SIGMA)[0] >= 1
                got.append(([bytes(d) for d in e.results_raw(0)], covs_bytes(e)))
            single[mode] = got
    monkeypatch.delenv("IRMV_SYNC_LAUNCH")
    assert single["graph"] == single["eager"]
    assert len({len(g[0]) for g in single["graph"]}) > 1                # the slots below differ in their counts
    with peng(wblob, num_slots=5, num_streams=2) as e:
        e.set_pose_cov(sigma_px=SIGMA)                                   # (in front of the yaw enable: the yaw launch goes in front)
        e.set_yaw_solve()
        for first, count in ((0, 5), (1, 2), (3, 2)):
            perm = [(s + first + count) % 5 for s in range(5)]
            for s in range(5):
                put(e, fr[perm[s]], s)
            e.submit(first, count)
            e.wait_slots(first, count)
            for s in range(first, first + count):
                n1, ny = check_slot(e, s, SIGMA)
                assert n1 >= 1 and ny >= 1
                assert ([bytes(d) for d in e.results_raw(s)], covs_bytes(e, s)) == single["graph"][perm[s]], (first, count, s)
        e.set_up((0.1, -1.0, 0.2), 1)
        e.submit(0, 5)
        e.wait()
        for s in range(5):
            assert check_slot(e, s, SIGMA)[1] >= 1
        assert covs_bytes(e, 1) != single["graph"][1][1]                 # (slot 1 holds frame 1 again) its own up vector


def test_window_engine_equals_the_plain_engine_on_the_crop_across_a_move_and_in_the_frame_view(wblob):
    frame = frame_of(16)
    want = {}
    for org in ((3, 70), (60, 2)):
        with peng(wblob, camera_matrix=window.shifted_camera(K, org[0], org[1])) as p:
            p.set_yaw_solve()
            p.set_pose_cov(sigma_px=SIGMA)
            put(p, window.crop(frame, org[0], org[1], WIN[0], WIN[1], True))
            p.detect()
            want[org] = covs_bytes(p)
            assert sum(c.state == 1 for c in p.pose_covs(0)) >= 1
    with peng(wblob, src=FULL) as p:
        p.set_yaw_solve()
        p.set_pose_cov(sigma_px=SIGMA)
        put(p, frame)
        p.detect()
        want["frame"] = covs_bytes(p)
        assert check_slot(p, 0, SIGMA)[0] >= 1
    with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, camera_matrix=K) as w:
        w.set_yaw_solve()
        w.set_pose_cov(sigma_px=SIGMA)
        put(w, frame)
        for org in ((3, 70), (60, 2)):
            w.set_window(*org)
            w.detect()
            assert covs_bytes(w) == want[org], org
        w.set_view("frame")                                              # built behind the enable
        w.detect()
        assert covs_bytes(w) == want["frame"]


def test_tiled_step_records_by_tile_and_index(wblob):
    """One tiled step of two windows: each slot's records are, byte for byte, those of the ordinary step on the same window,
    and the record of merged record r is pose_covs(first + r.tile)[r.index]."""
    corners = [(0, 0), (66, 73)]
    frame = frame_of(12)
    with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, num_slots=3, camera_matrix=K) as e:
        e.set_yaw_solve()
        e.set_pose_cov(sigma_px=SIGMA)
        for s in range(3):
            put(e, frame, s)
        e.set_tiles(corners, 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        recs, _ = e.tile_results_raw(1)
        tiled = [([bytes(d) for d in e.results_raw(1 + t)], covs_bytes(e, 1 + t)) for t in range(2)]
        cs = [e.pose_covs(1 + t) for t in range(2)]
        assert len(recs) >= 1
        solved = 0
        for r in recs:
            assert bytes(r.det) == tiled[r.tile][0][r.index]
            c = cs[r.tile][r.index]
            assert (c.state != 0) == bool(r.det.pnp_ok == 1 and r.det.armor_valid == 1)
            solved += c.state == 1
        assert solved >= 1
        for t in range(2):
            e.submit(1 + t, 1)
            e.wait_slots(1 + t, 1)
            assert ([bytes(d) for d in e.results_raw(1 + t)], covs_bytes(e, 1 + t)) == tiled[t]


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_classical_and_refined_point_sources(blob, source):
    """The eight-plate scene of the refined tests as a whole step: the op stands behind the light extraction and reads the
    points it reports.  (The classical pairing finds no armor in this scene's boxes: its records are all state 0.)"""
    sblob = rc.step_blob(blob)
    img, _ = rc.step_scene()
    cam = ys.camera_of(DEFAULT_CAMERA_MATRIX, DEFAULT_DIST_COEFFS)
    with YoloEngine(None, rc.SRC, weights_blob=sblob, net_size=rc.NET[0], net_height=rc.NET[1], point_source=source) as e:
        e.set_yaw_solve()
        e.set_pose_cov(sigma_px=SIGMA)
        put(e, rc.to_buffer(img, True))
        e.detect()
        assert len(e.results_raw(0)) >= 4
        n1, _ = check_slot(e, 0, SIGMA, cam=cam)
        assert source == capi.POINTS_CLASSICAL or n1 >= 4
        names = [k["name"] for k in e.profile(0, 1)]
        assert names.index("pose_cov") == names.index("yaw_solve") + 1 == len(names) - 1


@pytest.mark.parametrize("yaw", [False, True], ids=["yaw-off", "yaw-on"])
def test_classical_engine_on_drawn_plates(blob, yaw):
    """OP_POSECOV behind OP_LIGHT on records the light extraction SOLVED: zoo poses drawn as two bright bars with one box
    around them (the recipe of tests/test_gpu_yaw_solve.py test_classical_engine_solves_drawn_plates), run_post on a classical
    engine.  Every record is the reference's on the four points and the pose the extraction reports; at least two have
    state 1."""
    import pose_prior_set as L
    import yaw_set as YS
    from oracle import oracle
    from test_gpu_pnp import _draw_bar
    from test_gpu_pose_prior import _box_head
    src = (1280, 1024)
    done = solved = yaws = 0
    with YoloEngine(None, src, weights_blob=blob, net_size=NET[0], net_height=NET[1], armor_size=L.SIZE, camera_matrix=YS.K,
                    dist_coeffs=list(YS.D), rotate180=False, point_source=capi.POINTS_CLASSICAL) as e:
        if yaw:
            e.set_yaw_solve()
        e.set_pose_cov(sigma_px=SIGMA)
        for c in P.zoo():
            if done >= 6:
                break
            q = c["pts"].astype(np.float64)
            if c["cam"] != L.CAM or c["size"] != L.SIZE or c["R"] is None or q[:, 0].min() < 60 or q[:, 0].max() > 1220 or q[:, 1].min() < 60 or q[:, 1].max() > 964:
                continue
            ll, lr = np.linalg.norm(q[1] - q[0]), np.linalg.norm(q[3] - q[2])
            if min(ll, lr) < 14 or max(ll, lr) > 300:
                continue
            img = np.zeros((src[1], src[0], 3), np.uint8)
            _draw_bar(img, q[0], q[1], 0.2 * ll)
            _draw_bar(img, q[3], q[2], 0.2 * lr)
            put(e, img)
            e.detect()                                     # the frame into the slot's device frame
            e.write_head(_box_head(e, src, q), 0)
            e.run_post(0, 1)
            dets = e.results_raw(0)
            assert len(dets) == 1
            if not oracle.extract_armor(img, np.array(dets[0].xyxy, np.float32))["ok"] or not dets[0].pnp_ok:
                continue
            assert dets[0].armor_valid == 1
            n1, ny = check_slot(e, 0, SIGMA, cam=YS.CAM)
            assert n1 == 1, c["name"]
            solved += n1
            yaws += ny
            done += 1
    assert done >= 4 and solved >= 2 and (yaws >= 1) == yaw


# ---- 4. liveness ------------------------------------------------------------------------------------------------------------------
def test_sigma_is_live_and_disable_zeroes(wblob):
    with peng(wblob) as e:
        e.set_pose_cov(sigma_px=1.0)
        put(e, win_frame(12))
        e.detect()
        g0 = e.debug_graph_count()
        one = e.pose_covs(0)
        assert check_slot(e, 0, 1.0)[0] >= 1
        e.set_pose_cov(sigma_px=2.0)
        e.detect()
        assert e.debug_graph_count() == g0
        two = e.pose_covs(0)
        assert check_slot(e, 0, 2.0)[0] >= 1                             # the exact ratio the reference gives: its own bits at 2.0
        k = next(i for i, c in enumerate(one) if c.state == 1)
        assert np.allclose(np.array(list(two[k].cov)), 4.0 * np.array(list(one[k].cov)), rtol=1e-12, atol=0)
        with pytest.raises(capi.IrmvError):
            e.set_pose_cov(sigma_px=65.0)
        assert e.pose_cov() == dict(enable=True, sigma_px=2.0)
        n = len(two)
        e.set_pose_cov(enable=False, sigma_px=2.0)
        assert covs_bytes(e) == [ZERO] * n                               # zeroed at once ...
        e.detect()
        assert covs_bytes(e) == [ZERO] * n and e.debug_graph_count() == g0   # ... and no step writes one
        e.set_pose_cov(sigma_px=2.0)
        assert covs_bytes(e) == [ZERO] * n                               # re-enabled: nothing of the earlier step
        e.detect()
        assert covs_bytes(e) == [bytes(c) for c in two] and e.debug_graph_count() == g0


# ---- 5. non-interference ------------------------------------------------------------------------------------------------------
def _everything(e, slot=0):
    return dict(dets=[bytes(d) for d in e.results_raw(slot)], alts=[bytes(a) for a in e.pose_alts(slot)],
                yaws=[bytes(y) for y in e.yaw_poses(slot)], patches=[bytes(p) for p in e.plate_patches(slot)],
                numbers=[bytes(n) for n in e.plate_numbers(slot)])


def test_the_other_records_do_not_notice(wblob):
    """irmv_det, alts, yaw poses, patches and numbers of an engine with the feature on against one that never enabled it:
    detect() and a batched submit, the plan nms, yaw, pose_cov, patch, number."""
    fr = [win_frame(30 + i) for i in range(3)]

    def mk(on):
        e = peng(wblob, num_slots=3)
        e.set_pose_prior(None)
        e.set_yaw_solve()
        if on:
            e.set_pose_cov(sigma_px=SIGMA)
        e.set_patches()
        e.set_number_model(TN.model())
        e.set_numbers(True)
        return e

    with mk(False) as never, mk(True) as e:
        for x in (never, e):
            for s in range(3):
                put(x, fr[s], s)
            x.detect(0)
        assert _everything(e) == _everything(never) and len(_everything(e)["dets"]) >= 1
        assert any(any(b) for b in _everything(e)["patches"]) and check_slot(e, 0, SIGMA)[0] >= 1
        assert any(n.state == 1 for n in e.plate_numbers(0)) and any(any(b) for b in _everything(e)["numbers"])
        for x in (never, e):
            x.submit(0, 3)
            x.wait()
        for s in range(3):
            assert _everything(e, s) == _everything(never, s)
        # the launch stands behind the yaw launch and in front of the patches, the numbers directly behind those
        names = [k["name"] for k in e.profile(0, 1)]
        i = names.index("pose_cov")
        assert names[i - 1:i + 3] == ["yaw_solve", "pose_cov", "plate_patch", "plate_number"], names[i - 1:]
        kinds = [o.kind.decode() for o in MR.graph_ops(e)]
        assert kinds[-4:] == ["yaw", "pose_cov", "patch", "number"] and "?" not in kinds
        assert "pose_cov" not in [k["name"] for k in never.profile(0, 1)]


def test_tile_records_do_not_notice(wblob):
    frame = frame_of(12)

    def go(on):
        with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, num_slots=3, camera_matrix=K) as e:
            if on:
                e.set_pose_cov(sigma_px=SIGMA)
            for s in range(3):
                put(e, frame, s)
            e.set_tiles([(0, 0), (66, 73)], 1)
            e.submit_tiles(0, 1, 2)
            e.wait_slots(1, 2)
            return [bytes(r) for r in e.tile_results_raw(1)[0]]

    a = go(False)
    assert len(a) >= 1 and go(True) == a


def test_a_never_enabled_engine_is_the_recorded_one(wblob, monkeypatch):
    """tests/golden/engine_registry.json holds the op list, the classified ranges, the graph count and the profile rows of
    this engine as the library of the commit in front of this feature built it (tests/golden/make_engine_registry.py): an engine
    that never enables the feature is that engine, and enabling adds one op, two ranges and one row to it."""
    import json
    import os
    from conftest import ROOT
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_registry.json")))
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_HEAD", "0")
    with peng(wblob) as e:
        put(e, win_frame(12))
        e.detect()
        ops = [[o.kind.decode(), o.kname.decode()] for o in MR.graph_ops(e)]
        allocs = [[a["name"], a["cls"], a["bytes"]] for a in e.debug_allocs()]
        assert ops == want["ops"]
        assert allocs == want["allocs"]
        assert [k["name"] for k in e.profile(0, 1)] == want["profile"]
        if e.sync_launch == want["sync_launch"]:         # (detect()'s launch form is chosen by timing at creation)
            assert e.debug_graph_count() == want["graph_count"]
        g = e.debug_graph_count()
        e.set_pose_cov()
        assert e.debug_graph_count() == 0                                # dropped once ...
        e.detect()
        assert e.debug_graph_count() == g                                # ... and captured again, as many
        assert [[o.kind.decode(), o.kname.decode()] for o in MR.graph_ops(e)] == want["ops"] + [["pose_cov", "pose_cov"]]
        added = [a for a in ([a["name"], a["cls"], a["bytes"]] for a in e.debug_allocs()) if a not in want["allocs"]]
        assert sorted(added) == [["posecov_dev", "SCRATCH", 288 * e.max_det], ["posecov_table", "CONST", 16]]
        assert [k["name"] for k in e.profile(0, 1)] == want["profile"] + ["pose_cov"]


# ---- 6. memory residue --------------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_what_device_memory_held(wblob):
    def go(fill):
        with peng(wblob) as e:
            e.set_yaw_solve()
            e.set_pose_cov(sigma_px=SIGMA)
            names = {r["name"]: r["cls"] for r in e.debug_allocs()}
            assert names["posecov_dev"] == "SCRATCH" and names["posecov_table"] == "CONST"
            if fill is not None:
                assert e.debug_fill_mem(fill) > 0
            put(e, win_frame(12))
            e.detect()
            return MR.freeze([e.results_raw(0), e.yaw_poses(0), e.pose_covs(0)])

    fresh = go(None)
    for pattern in MR.PATTERNS[1:]:
        assert go(pattern) == fresh
