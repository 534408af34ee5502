"""The oracle's light extraction, stage by stage, on the shape zoo (tests/light_shapes.py) against independent
statements in scipy / numpy / fp64 -- and the zoo's own power: it tells the classic wrong variants apart.

OpenCV is not available to pin the oracle (oracle/orc_light.c, PARITY UNPINNED), so these statements are what the
GPU-equals-oracle tests of tests/test_gpu_light_shapes.py rest on."""
import functools
import os

import numpy as np
from scipy import ndimage
from scipy.spatial import ConvexHull

import light_shapes as ls
from irmv_detection_amd import _build, capi
from oracle import oracle

S8 = np.ones((3, 3), bool)
MARGIN = 1e-9     # relative distance every gated quantity keeps from its limit (the device's atan2 may round differently)


@functools.lru_cache(maxsize=None)
def limits():
    if not os.path.exists(capi.lib_path()):
        _build.build()
    return capi.light_limits()


@functools.lru_cache(maxsize=None)
def zoo():
    z = ls.build_zoo(lds_image=limits()["lds_image"])
    ls.finish_point_caps(z, lambda m: len(oracle.scan_external(m.astype(np.uint8))[1]))
    return z


@functools.lru_cache(maxsize=16)
def zoo_image(f):
    return zoo().image(f)


def stages(case, params=None, image=None):
    """Every stage of the oracle on one zoo box: ROI, binary image, contours in discovery order, a light record per
    contour of 5 or more points, the armor."""
    P = params or oracle.light_params()
    img = zoo_image(case.frame) if image is None else image
    ok, roi, mn = oracle.light_roi(ls.W, ls.H, case.box)
    st = dict(case=case, roi_ok=ok, roi=roi, min_xy=mn, final=oracle.extract_armor(img, case.box, P))
    if not ok:
        return st
    st["bin"] = b = oracle.light_binary(img, roi, P.binary_threshold)
    st["starts"], st["points"] = s, p = oracle.scan_external(b)
    st["recs"] = [oracle.contour_light(p[s[i]:s[i + 1]], P, mn) if s[i + 1] - s[i] >= 5 else None for i in range(len(s) - 1)]
    return st


@functools.lru_cache(maxsize=None)
def all_stages():
    return [stages(c) for c in zoo().cases]


def fill(b):
    return ndimage.binary_fill_holes(b > 0)


# ---- part 3: the oracle against independent statements --------------------------------------------------------------
def test_zoo_is_what_it_claims():
    z, L = zoo(), limits()
    groups = {c.group for c in z.cases}
    assert groups == {"topology", "scan", "roi", "big", "caps", "gate", "threshold", "random"}
    assert sum(c.group == "random" for c in z.cases) >= 300 and len(z.cases) >= 700
    by = {(c.group, c.name): st for c, st in zip(z.cases, all_stages())}
    # caps: exactly on and one past each limit
    for n in (1023, 1024, 1025):
        assert len(by["caps", f"contours_{n}"]["starts"]) - 1 == n
    for n in (4095, 4096, 4097):
        st = by["caps", f"points_{n}"]
        assert len(st["points"]) == n and len(st["starts"]) - 1 <= L["max_contours"]
    assert L["max_contours"] == 1024 and L["points_cap"] == 4096
    # label images on both sides of the LDS limit
    for name, lds in (("lds_sq", True), ("pool_sq", False), ("lds_rect", True), ("pool_rect", False)):
        _, _, rw, rh = by["roi", name]["roi"]
        assert (ls.label_bytes(rw, rh) <= L["lds_image"]) == lds
    # big contours: the global-memory contour path, hulls of more than 64 and of more than 128 edges
    n_pts = {k[1]: max(np.diff(st["starts"])) for k, st in by.items() if k[0] == "big"}
    edges = {k[1]: max([r.hull_edges for r in st["recs"] if r], default=0) for k, st in by.items() if k[0] == "big"}
    assert n_pts["disc150"] > L["lds_points"] and n_pts["ellipse420x330"] > L["lds_points"] and n_pts["staircase"] > L["lds_points"]
    assert 64 < edges["disc150"] <= 128 < edges["ellipse420x330"]
    assert edges["square"] == 0 and edges["diamond"] == 0       # four contour points: never measured; the notched ones are
    assert edges["square_notch"] == 4 and edges["diamond_notch"] == 4 and edges["gon128"] > 64
    # scan geometry: starts on the asked padded columns
    for c in ls.SCAN_COLUMNS:
        st = by["scan", f"scan_out_{c}"]
        assert (c - 1) in st["points"][st["starts"][:-1], 0]
    # gate and merge: every pair of residues of the last two gated contours modulo 4; 0, 1, 2 lights
    pairs, totals = set(), set()
    for k, st in by.items():
        if k[0] == "gate":
            g = [i for i, r in enumerate(st["recs"]) if r and r.ok]
            totals.add(len(g))
            if len(g) >= 2:
                pairs.add((g[-1] % 4, g[-2] % 4))
    assert pairs == {(a, b) for a in range(4) for b in range(4)} and {0, 1, 2, 9} <= totals


def test_only_the_caps_group_exceeds_a_limit():
    L = limits()
    for st in all_stages():
        c = st["case"]
        if not st["roi_ok"]:
            assert c.cap is None
            continue
        over = len(st["starts"]) - 1 > L["max_contours"] or len(st["points"]) > L["points_cap"]
        assert over == (c.cap in ("contours", "points")), (c.name, len(st["starts"]) - 1, len(st["points"]))
        assert c.group == "caps" or c.cap is None


def test_gated_quantities_keep_their_distance_from_the_limits():
    """Where a correct kernel could differ from the oracle: tilt comes from atan2, which the device's math library need
    not round as glibc does.  No zoo contour sits within 1e-9 (relative) of a gate, no armor of a distance limit."""
    P = oracle.light_params()
    far = lambda v, lim: not np.isfinite(v) or abs(v - lim) > MARGIN * abs(lim)
    n = 0
    for st in all_stages():
        lights = [r for r in st.get("recs", []) if r]
        for r in lights:
            assert far(r.tilt, P.light_max_angle) and far(r.ratio, P.light_min_ratio) and far(r.ratio, P.light_max_ratio), st["case"].name
            n += 1
        ok = [r for r in lights if r.ok]
        if len(ok) >= 2:
            cd = oracle.armor_from_lights(ok[-1], ok[-2], P)["cd"]
            for lim in (P.armor_min_small_center_distance, P.armor_max_small_center_distance, P.armor_min_large_center_distance,
                        P.armor_max_large_center_distance):
                assert far(cd, lim), st["case"].name
    assert n > 1000


def _walk(c):
    """pixels on the closed polygon of a contour and its segment directions; every segment is one of the eight directions"""
    if len(c) == 1:
        return {tuple(c[0])}, []
    px, dirs = set(), []
    for a, b in zip(c, np.roll(c, -1, 0)):
        d = b.astype(int) - a
        n = int(np.abs(d).max())
        assert n > 0 and (d[0] == 0 or d[1] == 0 or abs(d[0]) == abs(d[1])), (a, b)
        u = d // n
        dirs.append(tuple(u))
        px.update((int(a[0] + k * u[0]), int(a[1] + k * u[1])) for k in range(n))
    return px, dirs


def test_contours_are_the_outer_borders_of_the_hole_filled_components():
    n_contours = 0
    for st in all_stages():
        if not st["roi_ok"]:
            continue
        name, b, s, p = st["case"].name, st["bin"], st["starts"], st["points"]
        filled = fill(b)
        lab, n = ndimage.label(filled, structure=S8)
        assert len(s) - 1 == n, name
        # raster order of each component's topmost-leftmost pixel = discovery order (the oracle returns the reverse)
        flat = lab.ravel()
        first = np.full(n + 1, flat.size)
        np.minimum.at(first, flat, np.arange(flat.size))
        order = np.argsort(first[1:]) + 1
        padded = np.pad(filled, 1)
        outside4 = ~(padded[:-2, 1:-1] & padded[2:, 1:-1] & padded[1:-1, :-2] & padded[1:-1, 2:])
        for i in range(n):
            c = p[s[i]:s[i + 1]]
            comp = order[i]
            assert (int(c[0][1]) * b.shape[1] + int(c[0][0])) == first[comp], name       # found at its first pixel, in raster order
            px, dirs = _walk(c)
            ys, xs = np.nonzero((lab == comp) & outside4) if n > 1 else np.nonzero(filled & outside4)
            assert px == set(zip(xs.tolist(), ys.tolist())), (name, i)
            assert all(d0 != d1 for d0, d1 in zip(dirs, dirs[1:] + dirs[:1])), (name, i)   # no collinear-redundant point
        n_contours += n
        cv = oracle.find_external_contours(b)                                              # OpenCV's order: last found first
        assert len(cv) == n and all(np.array_equal(cv[n - 1 - i], p[s[i]:s[i + 1]]) for i in range(n)), name
    assert n_contours > 5000


def _edge_areas(hull):
    """area of the bounding rectangle aligned with every hull edge, in the oracle's own operations (elementwise fp64)"""
    h = hull.astype(np.float64)
    out = []
    for i in range(len(h)):
        a, b = h[i], h[(i + 1) % len(h)]
        ux, uy = b[0] - a[0], b[1] - a[1]
        ln = np.sqrt(ux * ux + uy * uy)
        ux, uy = ux / ln, uy / ln
        dx, dy = h[:, 0] - a[0], h[:, 1] - a[1]
        sv, tv = dx * ux + dy * uy, -dx * uy + dy * ux
        out.append(((sv.max() - sv.min()) * (tv.max() - tv.min()), (a, ux, uy, sv.min(), sv.max(), tv.min(), tv.max())))
    return out


def _corners(rec):
    a, ux, uy, smin, smax, tmin, tmax = rec
    sx, tx = (smin, smax, smax, smin), (tmin, tmin, tmax, tmax)
    return np.array([[a[0] + sx[q] * ux - tx[q] * uy, a[1] + sx[q] * uy + tx[q] * ux] for q in range(4)]).astype(np.float32)


def _check_rect(pts):
    c, hull, chosen = oracle.min_area_rect_ex(pts)
    assert np.array_equal(c, oracle.min_area_rect(pts))
    cd = c.astype(np.float64)
    area = np.linalg.norm(cd[1] - cd[0]) * np.linalg.norm(cd[2] - cd[1])
    # brute force over the edges of scipy's hull, fp64 (the statement of tests/test_oracle_light.py)
    hv = pts[ConvexHull(pts.astype(float)).vertices].astype(float)
    best = np.inf
    for i in range(len(hv)):
        u = hv[(i + 1) % len(hv)] - hv[i]
        u /= np.linalg.norm(u)
        s, t = (hv - hv[i]) @ u, (hv - hv[i]) @ np.array([-u[1], u[0]])
        best = min(best, (s.max() - s.min()) * (t.max() - t.min()))
    assert abs(area - best) <= 1e-3 * max(best, 1.0)
    assert len(hull) == len(hv) and {tuple(v) for v in hull.tolist()} == {tuple(v) for v in hv.astype(int).tolist()}
    e0, e1 = cd[1] - cd[0], cd[3] - cd[0]
    a, b = (pts - cd[0]) @ e0 / max(e0 @ e0, 1e-12), (pts - cd[0]) @ e1 / max(e1 @ e1, 1e-12)
    assert a.min() >= -1e-4 and a.max() <= 1 + 1e-4 and b.min() >= -1e-4 and b.max() <= 1 + 1e-4
    # ties: the first minimal edge in hull order
    areas = _edge_areas(hull)
    first = int(np.argmin([a for a, _ in areas]))
    assert chosen == first and np.array_equal(_corners(areas[first][1]), c)
    return len(hull), sum(a == areas[first][0] for a, _ in areas)


def test_min_area_rect_on_big_hulls_and_ties():
    by = {c.name: st for c, st in zip(zoo().cases, all_stages()) if c.group in ("big", "gate")}
    most, ties = 0, {}
    for name, st in by.items():
        for i, r in enumerate(st["recs"]):
            if r and r.hull_edges:
                h, t = _check_rect(st["points"][st["starts"][i]:st["starts"][i + 1]])
                assert h == r.hull_edges
                most, ties[name] = max(most, h), t
    assert most > 128
    print("ties:", {k: v for k, v in ties.items() if v > 1})
    assert ties["square_cut"] == 4 and ties["square_notch"] == 4 and ties["diamond_notch"] == 4   # every edge ties; the first one must win
    # degenerate point sets, which no traced contour can be (see light_shapes): one point, two points, collinear, duplicates
    for pts, exp in (([[3, 4]] * 5, [[3, 4]] * 4), ([[1, 1], [5, 3], [1, 1], [5, 3], [5, 3]], [[1, 1], [1, 1], [5, 3], [5, 3]]),
                     ([[0, 0], [2, 2], [4, 4], [6, 6], [8, 8], [3, 3]], [[0, 0], [0, 0], [8, 8], [8, 8]]),
                     ([[9, 0], [7, 0], [1, 0], [4, 0], [2, 0]], [[1, 0], [1, 0], [9, 0], [9, 0]])):
        c, hull, chosen = oracle.min_area_rect_ex(np.array(pts, np.int16))
        assert c.tolist() == exp and chosen == -1 and len(hull) <= 2
        assert oracle.contour_light(np.array(pts, np.int16)).hull_edges == 0


def test_extract_armor_is_the_first_two_gated_contours_in_opencv_order():
    P = oracle.light_params()
    n_valid = 0
    for st in all_stages():
        f = st["final"]
        if not st["roi_ok"]:
            assert not f["ok"] and f["n_lights"] == 0
            continue
        ok = [r for r in st["recs"][::-1] if r and r.ok]      # OpenCV order: last found first
        assert f["n_lights"] == len(ok), st["case"].name
        if len(ok) < 2:
            assert not f["ok"]
            continue
        a = oracle.armor_from_lights(ok[0], ok[1], P)
        l, r = (ok[0], ok[1]) if ok[0].center[0] < ok[1].center[0] else (ok[1], ok[0])
        cd = np.hypot(l.center[0] - r.center[0], l.center[1] - r.center[1]) / ((ok[0].length + ok[1].length) / 2)
        valid = (0.8 <= cd <= 3.2) or (3.2 < cd <= 5.5)
        assert f["ok"] == a["ok"] == valid and abs(cd - a["cd"]) <= 1e-12 * cd, st["case"].name
        if valid:
            n_valid += 1
            assert f["size"] == a["size"] == int(cd > 3.2)
            exp = np.array([list(l.bottom), list(l.top), list(r.top), list(r.bottom)], np.float32)
            assert np.array_equal(f["pts"], exp) and np.array_equal(a["pts"], exp), st["case"].name
    assert n_valid >= 10


def test_threshold_frame_ties_the_zoo_to_binary_threshold():
    z = zoo()
    thr = [(c, st) for c, st in zip(z.cases, all_stages()) if c.group == "threshold"]
    topo = {c.name: st for c, st in zip(z.cases, all_stages()) if c.group == "topology"}
    img = zoo_image(thr[0][0].frame)
    assert set(np.unique((img.astype(int) @ np.array([3735, 19235, 9798]) + (1 << 14)) >> 15)) == {150, 151}
    for c, st in thr:
        if c.name in topo:
            assert np.array_equal(st["bin"], topo[c.name]["bin"]) and np.array_equal(st["points"], topo[c.name]["points"])


# ---- part 5: the zoo tells the classic wrong variants apart ---------------------------------------------------------
def test_zoo_tells_the_classic_contour_bugs_apart():
    z = zoo()
    hit = {}
    P = oracle.light_params()
    S4 = ndimage.generate_binary_structure(2, 1)
    for st in all_stages():
        c = st["case"]
        if not st["roi_ok"]:
            continue
        b, s, p = st["bin"] > 0, st["starts"], st["points"]
        n = len(s) - 1
        if ndimage.label(fill(b), structure=S4)[1] != n:
            hit.setdefault("4-connectivity instead of 8", c.name)
        if ndimage.label(b, structure=S8)[1] != n:
            hit.setdefault("holes and nested components counted as external", c.name)
        if n >= 2 and not all(np.array_equal(a, q) for a, q in zip(oracle.find_external_contours(st["bin"]), [p[s[i]:s[i + 1]] for i in range(n)])):
            hit.setdefault("contours in found-first order", c.name)
        # >= instead of > at the threshold
        img = zoo_image(c.frame)
        rx, ry, rw, rh = st["roi"]
        gray = (img[ry:ry + rh, rx:rx + rw].astype(int) @ np.array([3735, 19235, 9798]) + (1 << 14)) >> 15
        assert np.array_equal(gray > P.binary_threshold, b)
        if not np.array_equal(gray >= P.binary_threshold, b) and ndimage.label(fill(gray >= P.binary_threshold), structure=S8)[1] != n:
            hit.setdefault(">= instead of > at the threshold", c.name)
        # rounding instead of truncation in the ROI
        x0, y0, x1, y1 = np.float32(c.box)
        mnx, mny, mxx, mxy = max(x0, np.float32(0)), max(y0, np.float32(0)), min(x1, np.float32(ls.W)), min(y1, np.float32(ls.H))
        assert (int(mnx), int(mny), int(mxx - mnx), int(mxy - mny)) == st["roi"]
        rr = (int(np.rint(mnx)), int(np.rint(mny)), int(np.rint(mxx - mnx)), int(np.rint(mxy - mny)))
        if rr != st["roi"] and rr[0] + rr[2] <= ls.W and rr[1] + rr[3] <= ls.H:
            b2 = z.masks[c.frame][rr[1]:rr[1] + rr[3], rr[0]:rr[0] + rr[2]]
            if b2.shape != b.shape or not np.array_equal(b2, b):
                hit.setdefault("rounding instead of truncation in the ROI", c.name)
        # last minimal hull edge instead of first
        for i, r in enumerate(st["recs"]):
            if r and r.hull_edges and c.group in ("big", "gate"):
                _, hull, chosen = oracle.min_area_rect_ex(p[s[i]:s[i + 1]])
                areas = _edge_areas(hull)
                last = max(k for k, (a, _) in enumerate(areas) if a == areas[chosen][0])
                if last != chosen and not np.array_equal(_corners(areas[last][1]), np.array(r.corners, np.float32).reshape(4, 2)):
                    hit.setdefault("last minimal hull edge instead of first", c.name)
    for k, v in hit.items():
        print(f"zoo power: '{k}' changes box {v}")
    assert set(hit) == {"4-connectivity instead of 8", "holes and nested components counted as external", "contours in found-first order",
                        ">= instead of > at the threshold", "rounding instead of truncation in the ROI", "last minimal hull edge instead of first"}
