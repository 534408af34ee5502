"""Pose ambiguity on the GPU (include/irmv_hip.h, "pose ambiguity"): irmv_pnp_solve2, the alt records of the three point
sources, the untouched default, and the tilt prior -- decided in the kernel, compared bit for bit with
irmv_detection_amd.pose_prior.select on the device's own two solutions.

Smallest shapes: a 128 x 64 net on a 1280 x 1024 source (the classical and refined cases: tests/refine_craft.py's 256 x 128
scene), heads injected with write_head + run_post (tests/pose_prior_set.py quad_head: 32 quads a frame).  The reference is
always fed the keypoints a step REPORTS, the float32 the solver saw.
"""
import ctypes as C

import numpy as np
import pytest

import detect_craft as dc
import pnp_ref as P
import pose_prior_set as L
import refine_craft as rc
from irmv_detection_amd import capi, pose_prior as pp
from irmv_detection_amd.engine import PnPSolver, YoloEngine

pytestmark = pytest.mark.gpu

SRC, NET = (1280, 1024), (128, 64)
_, K, D = P.CAMERAS[L.CAM]
PER = 32                                   # quads per injected frame (pose_prior_set.cells)


def eng(blob, **kw):
    kw.setdefault("camera_matrix", K)
    kw.setdefault("dist_coeffs", list(D))
    return YoloEngine(None, kw.pop("src", SRC), weights_blob=blob, net_size=NET[0], net_height=NET[1], armor_size=L.SIZE, **kw)


@pytest.fixture(scope="module")
def solver():
    s = PnPSolver(K, list(D))
    yield s
    s.close()


def run(e, quads, slot=0, src=SRC):
    head, _ = L.quad_head(e, src, quads)
    e.write_head(head, slot)
    e.run_post(slot, 1)
    d = e.results_raw(slot)
    assert len(d) == len(quads)
    return d


def kpts_of(d):
    return np.array([list(r.kpts) for r in d], np.float32).reshape(-1, 8)


def pose6(r):
    return np.array(list(r.rvec) + list(r.tvec))


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def check_against_solve2(dets, alts, solver, want_pick=None, where=""):
    """Every record and its alt against solve2 of the reported keypoints: the reported pose is entry `pick`, the alt the other
    entry, err / err_alt theirs, bit for bit; state 0 and an all-zero record where pnp_ok == 0.  want_pick(j, RA, errA, RB, errB)
    -> the expected choice (None: A everywhere).  -> the picks."""
    ok, alt_ok, r, t, err = solver.solve_generic(kpts_of(dets), L.SIZE)
    picks = []
    for j, (d, a) in enumerate(zip(dets, alts)):
        assert bool(d.pnp_ok) == bool(ok[j]), (where, j)
        if not d.pnp_ok:
            assert a.state == 0 and bytes(a) == bytes(capi.PoseAlt()), (where, j)
            picks.append(None)
            continue
        assert ok[j], (where, j)
        pick = 0
        if want_pick is not None and alt_ok[j]:
            pick = int(want_pick(j, P.matrix_of(r[j, 0]), err[j, 0], P.matrix_of(r[j, 1]), err[j, 1]))
        assert a.state == 1 + pick, (where, j, a.state, pick)
        assert same_bits(pose6(d), np.concatenate([r[j, pick], t[j, pick]])), (where, j)
        assert same_bits(pose6(a), np.concatenate([r[j, 1 - pick], t[j, 1 - pick]])), (where, j)
        assert same_bits([a.err, a.err_alt], [err[j, pick], err[j, 1 - pick]]), (where, j)
        assert bool(a.alt_ok) == bool(alt_ok[j]), (where, j)
        if a.alt_ok:                                       # the alt's quaternion is its rotation's
            q, qr = np.array(list(a.quat)), P.quat_of(P.matrix_of(np.array(list(a.rvec))))
            assert min(np.abs(q - qr).max(), np.abs(q + qr).max()) <= P.BAR, (where, j)
        picks.append(pick)
    return picks


def zoo_quads(n, first=0):
    """Zoo quads with the hard groups (degenerate quads, near-pi, fronto-parallel) first."""
    Z = P.zoo()
    order = sorted(range(len(Z)), key=lambda i: (Z[i]["group"] == "random", i % 7, i))
    return [Z[i]["pts"] for i in order[first:first + n]]


# ---- 1. irmv_pnp_solve2 over the zoo ---------------------------------------------------------------------------------------
def test_solve2_over_the_zoo():
    Z = P.zoo()
    r64, rmp, cls = P.zoo_reference()
    stats = dict(n=0, degenerate=0, ambiguous=0, worst0=0.0, worst1=0.0)
    for cam in range(len(P.CAMERAS)):
        s = PnPSolver(P.CAMERAS[cam][1], list(P.CAMERAS[cam][2]))
        for size in (0, 1):
            idx = [i for i, c in enumerate(Z) if c["cam"] == cam and c["size"] == size]
            pts = np.stack([Z[i]["pts"].reshape(8) for i in idx])
            ok1, r1, t1 = s.solve_batch(pts, size)
            ok, alt_ok, r, t, err = s.solve_generic(pts, size)
            assert np.array_equal(ok, ok1.astype(bool)) and same_bits(r[:, 0], r1) and same_bits(t[:, 0], t1)      # entry 0 IS irmv_pnp_solve
            for j, i in enumerate(idx):
                b, c = rmp[i], cls[i]
                swapped = dict(b, R=b["R"][::-1], t=b["t"][::-1])
                R0 = P.matrix_of(r[j, 0]) if np.isfinite(r[j, 0]).all() else np.full((3, 3), np.nan)
                R1 = P.matrix_of(r[j, 1]) if np.isfinite(r[j, 1]).all() else np.full((3, 3), np.nan)
                p0, e0, _ = P.check(R0, t[j, 0], bool(ok[j]), b, c)
                p1, e1, _ = P.check(R1, t[j, 1], bool(ok[j] and alt_ok[j]), swapped, c)
                assert p0 and p1, (Z[i]["name"], e0, e1, c["bar"])
                if c["degenerate"]:
                    stats["degenerate"] += 1
                    continue
                assert ok[j] == b["ok"] and alt_ok[j], Z[i]["name"]
                assert np.isfinite(err[j]).all() and err[j, 0] <= err[j, 1], Z[i]["name"]                         # A first
                # (the ORDER is the reference's wherever it is not ambiguous: P.check above held entry 0 to the reference's
                # first solution and entry 1 to its second)
                stats["ambiguous"] += c["ambiguous"]
                stats["n"] += 1
                if not c["ill"]:
                    stats["worst0"], stats["worst1"] = max(stats["worst0"], e0), max(stats["worst1"], e1)
        s.close()
    print("irmv_pnp_solve2 over the zoo:", stats)
    assert stats["n"] + stats["degenerate"] == len(Z) and stats["worst1"] <= P.BAR


# ---- 2. the untouched default ----------------------------------------------------------------------------------------------
def test_default_is_untouched_keypoint(blob):
    """Before the first set_pose_prior, and after set_pose_prior(NULL): byte-identical irmv_det records on zoo heads; before it
    pose_alts is refused."""
    frames = [zoo_quads(PER, k * PER) for k in range(3)]
    with eng(blob) as e:
        before = [[bytes(d) for d in run(e, q)] for q in frames]
        n = C.c_int(0)
        buf = (capi.PoseAlt * e.max_det)()
        assert e._L.irmv_engine_pose_alts(e._h, 0, buf, e.max_det, C.byref(n)) == capi.ERR_ARG
        assert e.pose_prior()["mode"] == capi.POSE_MIN_ERR and e.pose_prior()["ratio"] == 8.0 and e.up().tolist() == [0.0, -1.0, 0.0]
        e.set_pose_prior(None)
        after = [[bytes(d) for d in run(e, q)] for q in frames]
        assert before == after
        assert len(e.pose_alts(0)) == PER
        failed = sum(d.pnp_ok == 0 for q in frames for d in run(e, q))
        e.set_pose_prior("prior", 8.0)                 # ... and MIN_ERR again after PRIOR
        e.set_pose_prior("min_err", 2.0, 0.5)
        assert [[bytes(d) for d in run(e, q)] for q in frames] == before
    assert failed >= 1                                 # the degenerate quads were among them


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_default_is_untouched_classical_and_refined(blob, source):
    """The eight-plate scene of the refined tests as a whole step: the records before set_pose_prior and after
    set_pose_prior(NULL) are byte-identical, and every solved record then has its alt (the scalar solver's)."""
    sblob = rc.step_blob(blob)
    img, _ = rc.step_scene()
    with YoloEngine(None, rc.SRC, weights_blob=sblob, net_size=rc.NET[0], net_height=rc.NET[1], point_source=source) as e:
        e.get_src_image_buffer()[:] = rc.to_buffer(img, True)
        e.detect()
        before = [bytes(d) for d in e.results_raw(0)]
        e.set_pose_prior(None)
        e.detect()
        dets = e.results_raw(0)
        alts = e.pose_alts(0)
        assert [bytes(d) for d in dets] == before and len(alts) == len(dets) >= 4
        # (the classical pairing finds no armor in this scene's boxes; its solved records are test_scalar_form_alts_equal_solve2's)
        assert source == capi.POINTS_CLASSICAL or sum(d.pnp_ok for d in dets) >= 4
        for d, a in zip(dets, alts):
            assert a.state == (1 if d.pnp_ok else 0) and (a.state == 1 or bytes(a) == bytes(capi.PoseAlt()))
        if source == capi.POINTS_REFINED:
            assert sum(d.reserved == 1 for d in dets) == 4      # the scene's refined count: those alts are the refined quads'


# ---- 3. the alt records are solve2's entry 1 ------------------------------------------------------------------------------
def test_pair_form_alts_equal_solve2(blob, solver):
    with eng(blob) as e:
        e.set_pose_prior(None)
        seen = dict(solved=0, failed=0)
        for k in range(4):
            dets = run(e, zoo_quads(PER, k * PER))
            picks = check_against_solve2(dets, e.pose_alts(0), solver, where=f"frame {k}")
            seen["solved"] += sum(p is not None for p in picks)
            seen["failed"] += sum(p is None for p in picks)
    print("pair form alts against solve2:", seen)
    assert seen["solved"] >= 100 and seen["failed"] >= 1


def _box_head(e, src, quad, logit=4.0):
    """One detection whose box holds the quad with a margin (integer DFL sides around the stride-8 cell at its centre)."""
    q = np.asarray(quad, np.float64).reshape(4, 2) * [NET[0] / src[0], NET[1] / src[1]]
    lo, hi = q.min(0) - 3.0, q.max(0) + 3.0
    ix, iy = int(q[:, 0].mean() // 8), int(q[:, 1].mean() // 8)
    cx, cy = (ix + 0.5) * 8, (iy + 0.5) * 8
    sides = [max(1, int(np.ceil(v / 8))) for v in (cx - lo[0], cy - lo[1], hi[0] - cx, hi[1] - cy)]
    assert 0 <= ix < NET[0] // 8 and 0 <= iy < NET[1] // 8 and all(1 <= s <= 15 for s in sides)
    no = e.head_channels
    nc = no - 64 - 8
    h = np.zeros((e.num_anchors, no), np.float32)
    h[:, :64] = dc.dfl_bias(0)
    h[:, 64:64 + nc] = dc.DARK
    a = iy * (NET[0] // 8) + ix
    for j, s in enumerate(sides):
        h[a, 16 * j:16 * j + 16] = dc.OFF_BIN
        h[a, 16 * j + s] = 0.0
    h[a, 64 + 2] = np.float32(logit)
    return h


def test_scalar_form_alts_equal_solve2(blob, solver):
    """The scalar solver's alt through a classical engine's step: zoo poses drawn as two bright bars (as
    test_gpu_pnp.test_light_form_on_zoo_poses draws them), a head with one box around them, run_post."""
    from oracle import oracle
    from test_gpu_pnp import _draw_bar
    done = 0
    with eng(blob, rotate180=False, point_source=capi.POINTS_CLASSICAL) as e0, eng(blob, rotate180=False, point_source=capi.POINTS_CLASSICAL) as e:
        e.set_pose_prior(None)
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
            dets = e.results_raw(0)
            assert len(dets) == 1
            if not oracle.extract_armor(img, np.array(dets[0].xyxy, np.float32))["ok"] or not dets[0].pnp_ok:
                continue
            assert dets[0].armor_valid == 1
            picks = check_against_solve2(dets, e.pose_alts(0), solver, where=c["name"])
            assert picks == [0]
            e0.get_src_image_buffer()[:] = img             # the untouched default of the classical source, on a solved record
            e0.detect()
            e0.write_head(_box_head(e0, SRC, q), 0)
            e0.run_post(0, 1)
            assert [bytes(d) for d in e0.results_raw(0)] == [bytes(d) for d in dets], c["name"]
            done += 1
    assert done >= 4


# ---- 4. mode PRIOR ------------------------------------------------------------------------------------------------------------
def _by_up(cases):
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault(c["u"].tobytes(), []).append(i)
    return [(np.frombuffer(k, np.float64), v) for k, v in groups.items()]


def test_prior_mode_over_the_lean_back_set(blob, solver):
    """state and the reported pose equal pose_prior.select on the device's own solve2 output, bit for bit, over the whole
    set.  On the margin cases -- B is the generating pose, the reference's rule picks it -- the reported pose is within BAR
    of the generating solution, where MIN_ERR (the engine until now) reports the mirror pose."""
    cases = L.lean_back_set()
    margin = {id(c) for c in L.margin_cases()}
    stats = dict(n=0, B=0, margin_right=0, margin_mirror_before=0)
    with eng(blob) as e:
        for u, idx in _by_up(cases):
            e.set_up(u)
            un = e.up()
            assert same_bits(un, pp.normalise_up(u))
            for k in range(0, len(idx), PER):
                part = [cases[i] for i in idx[k:k + PER]]
                quads = [c["pts"] for c in part]
                e.set_pose_prior("min_err")
                before = run(e, quads)
                check_against_solve2(before, e.pose_alts(0), solver, where="min_err")
                e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
                dets = run(e, quads)
                want = lambda j, RA, eA, RB, eB: pp.select(RA, eA, RB, eB, un, L.S, pp.DEFAULT_RATIO, pp.PRIOR)   # noqa: E731
                picks = check_against_solve2(dets, e.pose_alts(0), solver, want, where="prior")
                assert all(p is not None for p in picks)
                stats["n"] += len(picks)
                stats["B"] += sum(picks)
                for c, d0, d1 in zip(part, before, dets):
                    if id(c) not in margin:
                        continue
                    _, b, cl = L.reference(np.array(list(d1.kpts), np.float32))       # of the keypoints the step reports
                    g = L.mirror_index(b, c["R"])
                    e1 = P.pose_error(P.matrix_of(np.array(list(d1.rvec))), np.array(list(d1.tvec)), b["R"][g], b["t"][g])
                    e0 = P.pose_error(P.matrix_of(np.array(list(d0.rvec))), np.array(list(d0.tvec)), b["R"][g], b["t"][g])
                    assert d1.pnp_ok == 1 and e1 <= P.BAR, (e1, e0)                  # THE assertion: the generating pose is reported
                    stats["margin_right"] += 1
                    stats["margin_mirror_before"] += e0 > P.BAR
    print("PRIOR over the lean-back set:", stats)
    assert stats["n"] == len(cases) and stats["margin_right"] == len(margin) >= 30
    assert stats["margin_mirror_before"] >= 30           # ... and min-error reported the mirror pose there


# ---- 5. live and per slot -------------------------------------------------------------------------------------------------------
def test_two_slots_with_opposite_up_decide_oppositely(blob, solver):
    """One batched run_post of two slots with the same head: slot 0 with the scene's u reports B on the margin cases, slot 1
    with -u reports A.  set_up and a second set_pose_prior capture nothing anew."""
    u = L.margin_cases()[0]["u"]
    part = [c for c in L.margin_cases() if c["u"].tobytes() == u.tobytes()][:PER]
    assert len(part) >= 8

    def states(e, ups, ratio, s):
        """Both slots against the host rule with their own up vector -> their state lists."""
        out = []
        for slot, uu in enumerate(ups):
            un = e.up(slot)
            assert same_bits(un, pp.normalise_up(uu))
            want = lambda j, RA, eA, RB, eB: pp.select(RA, eA, RB, eB, un, s, ratio, pp.PRIOR)   # noqa: E731
            check_against_solve2(e.results_raw(slot), e.pose_alts(slot), solver, want, where=f"slot {slot}")
            out.append([a.state for a in e.pose_alts(slot)])
        return out

    with eng(blob, num_slots=2) as e:
        head, _ = L.quad_head(e, SRC, [c["pts"] for c in part])
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
        e.set_up(u, 0)
        e.set_up(-u, 1)
        for s in (0, 1):
            e.write_head(head, s)
        e.run_post(0, 2)
        g0 = e.debug_graph_count()
        st = states(e, (u, -u), pp.DEFAULT_RATIO, L.S)
        assert st[0] == [2] * len(part)                    # the scene's own up vector: B, the generating pose
        opposite = [j for j in range(len(part)) if st[1][j] == 1]
        assert len(opposite) >= 8                          # ... and the opposite one: A
        d = [e.results_raw(s) for s in (0, 1)]
        a = [e.pose_alts(s) for s in (0, 1)]
        for j in opposite:                                 # each slot's report is the other's alt
            assert same_bits(pose6(d[0][j]), pose6(a[1][j])) and same_bits(pose6(d[1][j]), pose6(a[0][j]))
        # live: swap the two vectors, change the prior; the same graph runs
        e.set_up(-u, 0)
        e.set_up(u, 1)
        e.set_pose_prior("prior", 4.0, L.S)
        e.run_post(0, 2)
        assert e.debug_graph_count() == g0
        assert states(e, (-u, u), 4.0, L.S) == [st[1], st[0]]
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, -L.S)  # the outpost's tilt
        e.run_post(0, 2)
        assert e.debug_graph_count() == g0
        states(e, (-u, u), pp.DEFAULT_RATIO, -L.S)
        with pytest.raises(capi.IrmvError):
            e.set_up((0.0, 0.0, 0.0), 0)
        with pytest.raises(capi.IrmvError):
            e.set_pose_prior("prior", 0.5)
        assert same_bits(e.up(0), pp.normalise_up(-u)) and e.pose_prior()["ratio"] == pp.DEFAULT_RATIO


def test_window_move_and_frame_view_keep_the_decisions(blob):
    """A window engine: the same full-frame quads before and after a window move, and in the frame view -- the crop only moves
    the principal point, u is untouched: the same states, and poses and alts equal up to what the keypoints' float32 rounding
    does to them.  That bound: a keypoint below 2048 px has an ulp of 2^-13 px and goes through four roundings (logit, decode,
    scale, shift): <= 5e-4 px; on this set 0.5 px of noise moves a pose by less than 1 (rad, m), so 2 per px is generous:
    1e-3.  The decisions themselves have a cost gap of >= 0.1 by construction and must not move at all."""
    FULL, WIN = (322, 201), (256, 128)
    u = L.margin_cases()[0]["u"]
    part = ([c for c in L.margin_cases() if c["u"].tobytes() == u.tobytes()][:12] +
            [c for c in L.lean_back_set() if c["kept"] and not c["pick"] and c["u"].tobytes() == u.tobytes()][:12])
    quads = [c["pts"].astype(np.float64) for c in part]
    snaps = []
    with YoloEngine(None, FULL, weights_blob=blob, net_size=NET[0], net_height=NET[1], window=WIN, camera_matrix=K, dist_coeffs=list(D),
                    armor_size=L.SIZE, rotate180=False) as e:
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
        e.set_up(u)
        for view, org in (("window", (0, 0)), ("window", (66, 73)), ("window", (13, 40)), ("frame", (0, 0))):
            e.set_view(view)
            if view == "window":
                e.set_window(*org)
            src = WIN if view == "window" else FULL
            dets = run(e, [q - np.array(org, np.float64) for q in quads], src=src)
            alts = e.pose_alts(0)
            assert all(d.pnp_ok for d in dets)
            snaps.append((np.stack([pose6(d) for d in dets]), np.stack([pose6(a) for a in alts]), [a.state for a in alts]))
    assert snaps[0][2].count(2) >= 8 and snaps[0][2].count(1) >= 8
    for s in snaps[1:]:
        assert s[2] == snaps[0][2]
        assert np.abs(s[0] - snaps[0][0]).max() <= 1e-3 and np.abs(s[1] - snaps[0][1]).max() <= 1e-3


def test_tiled_step_alts_by_tile_and_index(blob):
    """One tiled step of two windows: each slot's alts are, byte for byte, those of the ordinary step on the same window, and
    the alt of merged record r is pose_alts(first + r.tile)[r.index]."""
    from test_gpu_window import FULL, WIN, frame_of
    wblob = dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))
    corners = [(0, 0), (66, 73)]
    frame = frame_of(12)
    with YoloEngine(None, FULL, weights_blob=wblob, net_size=NET[0], net_height=NET[1], window=WIN, num_slots=3, camera_matrix=K) as e:
        e.set_pose_prior("prior", pp.DEFAULT_RATIO, L.S)
        for s in range(3):
            e.set_up((0.1, -1.0, 0.2), s)
            e.get_src_image_buffer(s)[:] = frame
        e.set_tiles(corners, 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        recs, _ = e.tile_results_raw(1)
        tiled = [([bytes(d) for d in e.results_raw(1 + t)], [bytes(a) for a in e.pose_alts(1 + t)]) for t in range(2)]
        alts = [e.pose_alts(1 + t) for t in range(2)]
        assert len(recs) >= 1
        solved = 0
        for r in recs:
            assert bytes(r.det) == tiled[r.tile][0][r.index]
            a = alts[r.tile][r.index]
            assert (a.state >= 1) == bool(r.det.pnp_ok)
            solved += a.state >= 1
        assert solved >= 1
        for t in range(2):                                 # the ordinary step of the same window on the same frame
            e.submit(1 + t, 1)
            e.wait_slots(1 + t, 1)
            assert [bytes(d) for d in e.results_raw(1 + t)] == tiled[t][0]
            assert [bytes(a) for a in e.pose_alts(1 + t)] == tiled[t][1]


# ---- 6. a bad keypoint in one record -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, 1e8, -1e8], ids=["nan", "2^24", "-2^24"])
def test_bad_keypoint_fails_one_record_only(blob, bad):
    u = L.margin_cases()[0]["u"]
    part = ([c for c in L.margin_cases() if c["u"].tobytes() == u.tobytes()][:6] +
            [c for c in L.lean_back_set() if c["kept"] and not c["pick"] and c["u"].tobytes() == u.tobytes()][:6])
    quads = [c["pts"] for c in part]
    with eng(blob) as e:
        e.set_pose_prior("prior", float("inf"), L.S)
        e.set_up(u)
        head, anchors = L.quad_head(e, SRC, quads)
        nc = e.head_channels - 64 - 8
        e.write_head(head, 0); e.run_post(0, 1)
        clean_d, clean_a = [bytes(d) for d in e.results_raw(0)], [bytes(a) for a in e.pose_alts(0)]
        assert all(d.pnp_ok for d in e.results_raw(0)) and {a.state for a in e.pose_alts(0)} == {1, 2}
        for hit, k in ((3, 0), (8, 5), (11, 7)):            # both lanes of the pair carry the bad point in turn
            dirty = head.copy()
            dirty[anchors[hit], 64 + nc + k] = bad
            e.write_head(dirty, 0); e.run_post(0, 1)
            d, a = e.results_raw(0), e.pose_alts(0)
            assert len(d) == len(quads) and d[hit].pnp_ok == 0 and a[hit].state == 0 and bytes(a[hit]) == bytes(capi.PoseAlt())
            for j in range(len(quads)):
                if j != hit:
                    assert bytes(d[j]) == clean_d[j] and bytes(a[j]) == clean_a[j], (hit, j)
