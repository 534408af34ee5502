"""The device PnP solvers on the pose zoo against the independent reference (tests/pnp_ref.py): the scalar form through
irmv_pnp_solve, the lane-pair form through write_head + run_post, and terms: pnp_ref.py and DESIGN.md section 5.
the scalar form's second compilation (light_extract_kernel) through irmv_engine_extract_armors of a classical engine."""
import collections

import numpy as np
import pytest

import pnp_ref as P
from irmv_detection_amd import capi
from irmv_detection_amd.engine import PnPSolver, YoloEngine

pytestmark = pytest.mark.gpu


def _check_batch(names, pts, ok, rvec, tvec, refs, stats):
    """Every solved quad against the mpmath reference.  refs[j] = (float64 run, mpmath run, classification) of quad j.
    -> [(j, mpmath run, classification, matched solution)] of the quads that are not degenerate."""
    live = []
    for j, (a, b, c) in enumerate(refs):
        R = P.matrix_of(rvec[j]) if np.isfinite(rvec[j]).all() else np.full((3, 3), np.nan)
        passed, err, which = P.check(R, tvec[j], bool(ok[j]), b, c)
        assert passed, (names[j], err, c["bar"], bool(ok[j]))
        if c["degenerate"]:
            stats["degenerate"] += 1
            continue
        assert bool(ok[j]) == b["ok"], names[j]
        stats["ambiguous"] += c["ambiguous"]
        stats["ill"] += c["ill"]
        stats["worst"] = max(stats["worst"], err if not c["ill"] else 0.0)
        if P.pi_gap(b["R"][which]) > 1e-3 and not c["ill"]:
            d = np.abs(rvec[j] - P.rvec_of(b["R"][which])).max()
            stats["worst_rvec"] = max(stats["worst_rvec"], d)
            assert d <= P.BAR, (names[j], d)
        elif not c["ill"]:
            stats["near_pi"] += 1
        stats["n"] += 1
        live.append((j, b, c, which))
    return live


_REF_CACHE = {}


def _reference(cam, size, pts):
    key = (cam, size, np.asarray(pts, np.float32).tobytes())
    if key not in _REF_CACHE:
        _, K, D = P.CAMERAS[cam]
        a = P.solve64(K, D, pts, size)
        b = P.solve_mp(K, D, pts, size, hnull=a["hnull"])
        _REF_CACHE[key] = (a, b, P.classify(a, b))
    return _REF_CACHE[key]


def _stats():
    return dict(n=0, degenerate=0, ambiguous=0, ill=0, near_pi=0, worst=0.0, worst_rvec=0.0)


def test_pnp_solve_whole_zoo():
    """irmv_pnp_solve: every case of the zoo with its camera and plate size."""
    Z = P.zoo()
    refs = P.zoo_reference()
    st = _stats()
    for cam in range(len(P.CAMERAS)):
        solver = PnPSolver(P.CAMERAS[cam][1], list(P.CAMERAS[cam][2]))
        for size in (0, 1):
            idx = [i for i, c in enumerate(Z) if c["cam"] == cam and c["size"] == size]
            pts = np.stack([Z[i]["pts"].reshape(8) for i in idx])
            ok, r, t = solver.solve_batch(pts, size)
            _check_batch([Z[i]["name"] for i in idx], pts, ok, r, t, [(refs[0][i], refs[1][i], refs[2][i]) for i in idx], st)
            for i, o in zip(idx, ok):
                if Z[i]["name"].endswith("coincident") and "two_" not in Z[i]["name"]:
                    assert o == 0, Z[i]["name"]
        solver.close()
    print("irmv_pnp_solve over the zoo:", st)
    assert st["n"] + st["degenerate"] == len(Z) and st["near_pi"] >= 100


def test_pnp_solve_non_finite_coordinates():
    """NaN and +-Inf in a single coordinate: ok = 0 for that armor, its neighbours in the batch bit-identical to a clean run."""
    Z = [c for c in P.zoo() if c["group"] == "random" and c["cam"] == 0 and c["size"] == 0][:130]
    pts = np.stack([c["pts"].reshape(8) for c in Z])
    solver = PnPSolver(P.CAMERAS[0][1], list(P.CAMERAS[0][2]))
    ok0, r0, t0 = solver.solve_batch(pts, 0)
    assert ok0.all()
    hit = np.arange(1, 130, 3)
    dirty = pts.copy()
    for n, j in enumerate(hit):
        dirty[j, n % 8] = (np.nan, np.inf, -np.inf)[n % 3]
    ok, r, t = solver.solve_batch(dirty, 0)
    solver.close()
    clean = np.setdiff1d(np.arange(130), hit)
    assert not ok[hit].any()
    assert ok[clean].all() and np.array_equal(r[clean], r0[clean]) and np.array_equal(t[clean], t0[clean])


def test_pnp_solve_huge_coordinate():
    """1e30 in a single coordinate -> ok = 0 for that armor, neighbours untouched.  1e30 overflows nothing in fp64 (the solver
    used to answer ok = 1 with a finite, meaningless pose): the solvers refuse a float32 coordinate that no longer resolves
    a pixel, |v| >= 2^24 (pnp_ref.PIXEL_LIMIT).  Both sides of that edge are checked on the undistorted camera."""
    Z = [c for c in P.zoo() if c["group"] == "random" and c["cam"] == 0 and c["size"] == 0][:64]
    pts = np.stack([c["pts"].reshape(8) for c in Z])
    for cam in (0, 1):
        solver = PnPSolver(P.CAMERAS[cam][1], list(P.CAMERAS[cam][2]))
        ok0, r0, t0 = solver.solve_batch(pts, 0)
        hit = np.arange(2, 64, 5)
        dirty = pts.copy()
        for n, j in enumerate(hit):
            dirty[j, n % 8] = (1e30, -1e30, P.PIXEL_LIMIT, -P.PIXEL_LIMIT)[n % 4]
        ok, r, t = solver.solve_batch(dirty, 0)
        clean = np.setdiff1d(np.arange(64), hit)
        print("1e30 / 2^24 in one coordinate: ok =", ok[hit].tolist())
        assert np.array_equal(r[clean], r0[clean]) and np.array_equal(t[clean], t0[clean]) and np.array_equal(ok[clean], ok0[clean])
        assert not ok[hit].any()
        if cam == 1:        # the last float32 below the limit is still solved, to the reference
            edge = pts[:8].copy()
            edge[np.arange(8), np.arange(8)] = np.float32(P.PIXEL_LIMIT - 1)
            ok, r, t = solver.solve_batch(edge, 0)
            for j in range(8):
                a, b, c = _reference(1, 0, edge[j])
                assert (c["degenerate"] or bool(ok[j]) == b["ok"]) and P.check(P.matrix_of(r[j]), t[j], bool(ok[j]), b, c)[0], j
        solver.close()


def test_pnp_solve_batch_sizes_on_one_solver():
    """0, 1, 63, 64, 65 and 3000 quads on ONE solver object, rising and then falling: the buffer regrowth and the reuse of a
    larger buffer both carry checked results."""
    Z = P.zoo()
    refs = P.zoo_reference()
    idx_all = [i for i, c in enumerate(Z) if c["cam"] == 0 and c["size"] == 1]
    solver = PnPSolver(P.CAMERAS[0][1], list(P.CAMERAS[0][2]))
    st = _stats()
    start = 0
    for n in (0, 1, 63, 64, 65, 3000, 65, 64, 63, 1, 0):
        idx = [idx_all[(start + k) % len(idx_all)] for k in range(n)]
        start += 37
        pts = np.stack([Z[i]["pts"].reshape(8) for i in idx]) if n else np.zeros((0, 8), np.float32)
        ok, r, t = solver.solve_batch(pts, 1)
        assert len(ok) == n
        _check_batch([Z[i]["name"] for i in idx], pts, ok, r, t, [(refs[0][i], refs[1][i], refs[2][i]) for i in idx], st)
    solver.close()
    assert st["n"] + st["degenerate"] == 2 * (1 + 63 + 64 + 65) + 3000


# engine configurations of the pair form: (source size, net width, net height, resize mode, plate size, camera)
PAIR_ENGINES = (
    ((1280, 1024), 640, None, capi.RESIZE_STRETCH, 0, 0),
    ((1280, 1024), 640, 512, capi.RESIZE_STRETCH, 1, 1),
    ((1280, 1024), 640, None, capi.RESIZE_LETTERBOX, 1, 2),
    ((1280, 720), 640, 512, capi.RESIZE_LETTERBOX, 0, 0),
    ((640, 640), 640, None, capi.RESIZE_STRETCH, 1, 3),        # identity scaling, power-of-two camera: exact zeros survive the decode
)
KEPT = (1, 2, 3, 99, 100, 255, 256)


def _pair_head(e, src, mode, quads):
    """A head that makes survivor j report (about) quads[j]: stride-8 anchors four cells apart with a 16 px box each (no
    two overlap, so NMS keeps all), distinct descending logits, keypoint logits v = (k / stride - ix) / 2."""
    nw, nh = e.net_width, e.net_height
    if mode == capi.RESIZE_STRETCH:
        sx, sy, ox, oy = nw / src[0], nh / src[1], 0.0, 0.0
    else:
        sx = sy = min(nw / src[0], nh / src[1])
        ox, oy = (nw - src[0] * sx) / 2, (nh - src[1] * sy) / 2
    W8 = nw // 8
    cells = [(ix, iy) for iy in range(2, nh // 8, 4) for ix in range(2, W8, 4)]
    assert len(cells) >= len(quads)
    head = np.zeros((e.num_anchors, e.head_channels), np.float32)
    head[:, 64:78] = -20.0
    head[:, 1:64:16] = 20.0                                   # every DFL side: bin 1
    anchors = []
    for j, q in enumerate(quads):
        ix, iy = cells[j]
        a = iy * W8 + ix
        head[a, 64 + j % 14] = 8.0 - 0.01 * j
        k = q.reshape(4, 2).astype(np.float64) * [sx, sy] + [ox, oy]
        head[a, 78:86] = ((k / 8 - [ix, iy]) / 2).reshape(8)
        anchors.append(a)
    return head, anchors


@pytest.mark.parametrize("cfg", PAIR_ENGINES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-net{c[1]}x{c[2] or c[1]}-mode{c[3]}-size{c[4]}-{P.CAMERAS[c[5]][0]}")
def test_pair_form_on_the_zoo(blob, cfg):
    """solve_pnp_ippe_pair at the tail of nms_pnp_kernel: zoo quads injected as keypoint logits, kept = 1 ... 256 of max_det =
    256 (first, last, odd and LDS-overlapping pairs).  The reference is fed the kpts the step REPORTS, the float32 the solver
    saw.  quat against the reference's, up to sign."""
    src, nw, nh, mode, size, cam = cfg
    Z = P.zoo()
    # the hard groups first, so that every kept count carries them; any quad is a legitimate input for any camera
    order = sorted((i for i, c in enumerate(Z) if c["size"] == size and (cam == 3 or c["cam"] in (cam, 3))),
                   key=lambda i: (Z[i]["group"] == "random", i % 7, i))
    st = _stats()
    branches, flags = collections.Counter(), collections.Counter()
    _, K, D = P.CAMERAS[cam]
    with YoloEngine(None, src, weights_blob=blob, net_size=nw, net_height=nh, resize_mode=mode, armor_size=size, max_det=256,
                    camera_matrix=K, dist_coeffs=list(D)) as e:
        start = 0
        for kept in KEPT:
            idx = [order[(start + k) % len(order)] for k in range(kept)]
            start += kept
            head, anchors = _pair_head(e, src, mode, [Z[i]["pts"] for i in idx])
            e.write_head(head, 0)
            e.run_post(0, 1)
            raw = e.read_raw(0)
            arm = e.results(0)
            assert raw["num_dets"] == kept == len(arm) and raw["anchors"].tolist() == anchors
            pts = np.stack([a.image_points().reshape(8) for a in arm]).astype(np.float32)
            ok = np.array([a.pnp_ok for a in arm]); r = np.stack([a.rvec for a in arm]); t = np.stack([a.tvec for a in arm])
            assert all(int(a.size) == size for a in arm)
            for j, b, c, which in _check_batch([Z[i]["name"] for i in idx], pts, ok, r, t, [_reference(cam, size, p) for p in pts], st):
                q, qr = arm[j].quat_xyzw, P.quat_of(b["R"][which])
                bar = c["bar"]
                assert min(np.abs(q - qr).max(), np.abs(q + qr).max()) <= bar, (Z[idx[j]]["name"], q, qr)
                branches[P.quat_branch(b["R"][which])] += 1
            for p in pts:
                flags.update(P.degenerate_flags(K, D, p, size))
    print(f"pair form {cfg}: {st}; rot_to_quat branches {dict(branches)}; degenerate flags {dict(flags)}")
    assert all(branches[b] >= 1 for b in ("trace", "x", "y", "z")), branches
    assert flags["den"] >= 1
    if cam == 3:
        assert flags["h8"] >= 1 and flags["t0"] >= 1


def test_pair_form_refuses_an_out_of_range_keypoint(blob):
    """A finite keypoint logit of 1e8 on one survivor decodes to a pixel beyond 2^24: pnp_ok = 0 for that survivor (each lane of
    the pair tests its own two points; the verdicts meet through the solver's shuffles), its neighbours bit-identical to a
    clean run.  Every keypoint slot in turn, so that both lanes of the pair carry the bad point."""
    Z = [c for c in P.zoo() if c["group"] == "random" and c["cam"] == 0 and c["size"] == 0][:5]
    src = (1280, 1024)
    with YoloEngine(None, src, weights_blob=blob, max_det=256) as e:
        head, anchors = _pair_head(e, src, capi.RESIZE_STRETCH, [c["pts"] for c in Z])
        e.write_head(head, 0); e.run_post(0, 1)
        clean = e.results(0)
        assert len(clean) == 5 and all(a.pnp_ok for a in clean)
        for k in range(8):
            dirty = head.copy()
            dirty[anchors[2], 78 + k] = 1e8 if k % 2 else -1e8
            e.write_head(dirty, 0); e.run_post(0, 1)
            arm = e.results(0)
            assert len(arm) == 5 and not arm[2].pnp_ok and abs(arm[2].image_points().reshape(8)[k]) >= P.PIXEL_LIMIT, k
            for j in (0, 1, 3, 4):
                assert arm[j].pnp_ok and np.array_equal(arm[j].rvec, clean[j].rvec) and np.array_equal(arm[j].tvec, clean[j].tvec)
                assert np.array_equal(arm[j].quat_xyzw, clean[j].quat_xyzw)


def _draw_bar(img, p0, p1, width):
    """A filled white rectangle of the given width around the segment p0 -> p1."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    d = p1 - p0
    L = np.linalg.norm(d)
    u = d / L
    lo = np.floor(np.minimum(p0, p1) - width).astype(int)
    hi = np.ceil(np.maximum(p0, p1) + width).astype(int) + 1
    ys, xs = np.mgrid[max(lo[1], 0):min(hi[1], img.shape[0]), max(lo[0], 0):min(hi[0], img.shape[1])]
    rx, ry = xs - p0[0], ys - p0[1]
    along, across = rx * u[0] + ry * u[1], -rx * u[1] + ry * u[0]
    img[ys[(along >= 0) & (along <= L) & (np.abs(across) <= width / 2)], xs[(along >= 0) & (along <= L) & (np.abs(across) <= width / 2)]] = 255


@pytest.mark.parametrize("cam,model", [(0, 0), (2, 1)])
def test_light_form_on_zoo_poses(blob, cam, model):
    """solve_pnp_ippe as compiled into light_extract_kernel, and its plate-size switch: zoo poses drawn as two bright bars
    between the projected corner pairs (LB-LT, RT-RB; width = a fifth of the length, inside the light gates), through
    irmv_engine_extract_armors of a classical engine.  The reference is fed the kpts the kernel REPORTS.  The plate model this
    kernel solves with is the ENGINE's `armor_size` (the reference solves every armor with one model, src/pnp_solver.cpp:47-48;
    k_light.hip `pnp_armor_size`), not the size the light gates classify: one engine per model; the classified size is reported
    in `armor_size`, must be the CPU oracle's, and both values must occur.
    Poses: those of the camera whose quad lies inside the frame with lights of >= 14 px and which the CPU oracle's light
    extraction accepts."""
    from oracle import oracle
    _, K, D = P.CAMERAS[cam]
    st = _stats()
    sizes = collections.Counter()
    with YoloEngine(None, (1280, 1024), weights_blob=blob, rotate180=False, point_source=capi.POINTS_CLASSICAL,
                    camera_matrix=K, dist_coeffs=list(D), armor_size=model) as e:
        for c in P.zoo():
            if st["n"] >= 40:
                break
            q = c["pts"].astype(np.float64)
            if c["cam"] != cam or c["R"] is None or q[:, 0].min() < 30 or q[:, 0].max() > 1250 or q[:, 1].min() < 30 or q[:, 1].max() > 994:
                continue
            ll, lr = np.linalg.norm(q[1] - q[0]), np.linalg.norm(q[3] - q[2])
            if min(ll, lr) < 14 or min(ll, lr) > 400:
                continue
            img = np.zeros((1024, 1280, 3), np.uint8)
            _draw_bar(img, q[0], q[1], 0.2 * ll)
            _draw_bar(img, q[3], q[2], 0.2 * lr)
            box = np.array([[q[:, 0].min() - 25, q[:, 1].min() - 25, q[:, 0].max() + 25, q[:, 1].max() + 25]], np.float32)
            o = oracle.extract_armor(img, box[0])
            if not o["ok"]:
                continue
            e.get_src_image_buffer()[:] = img
            a = e.extract_armors(box)[0]
            assert a.valid and not a.no_answer and int(a.size) == o["size"], c["name"]
            sizes[(c["size"], int(a.size))] += 1
            pts = a.image_points().reshape(1, 8).astype(np.float32)
            ref = _reference(cam, model, pts[0])
            for j, b, cl, which in _check_batch([c["name"]], pts, [a.pnp_ok], a.rvec[None], a.tvec[None], [ref], st):
                qr = P.quat_of(b["R"][which])
                assert min(np.abs(a.quat_xyzw - qr).max(), np.abs(a.quat_xyzw + qr).max()) <= cl["bar"], c["name"]
    print(f"light form, camera {P.CAMERAS[cam][0]}, plate model {model}: {st}; (drawn plate size, reported armor_size): {dict(sizes)}")
    assert st["n"] >= 24                                            # a few dozen poses per camera
    assert {r for _, r in sizes} == {0, 1}, sizes                   # the gates classify both sizes; the solve uses `model` for all
