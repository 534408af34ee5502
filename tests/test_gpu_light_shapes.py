"""light_extract_kernel against the oracle, stage by stage, on the shape zoo (tests/light_shapes.py) through the test
hook irmv_engine_light_trace: contour counts, start offsets and every contour point in discovery order; rectangle
corners, gate verdict, top / bottom / center / length bit for bit; the final Det; and `no answer` predicted from the
oracle's counts, never tolerated.  The oracle's own anchors are in tests/test_light_shapes.py.

Wall time on an MI355X, same machine, same run: this file 3.4 s (four engines; the longest test 1.1 s, which includes
the oracle's pass over the zoo), tests/test_gpu_light.py 1.8 s.  The latter was timed on this tree, whose production
launches are the parent commit's (the trace pointer is null); the parent's own build was not timed.  No test here takes
longer than that whole file, so none is named test_slow_.

Each test prints one line, e.g.
light zoo [classical engine, rotate180=1, slots 0 and 2]: boxes 1394, contours 27794, points 341778, lds_images 1350,
pool_images 44, lds_contours 9974, global_contours 152, hulls_over_64 12, second_chunk_starts 3184, armors 158,
no_answer 8, worst case none (every stage exact), 0.5 s"""
import time

import numpy as np
import pytest

import light_shapes as ls
from irmv_detection_amd import capi
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_light_shapes import all_stages, limits, zoo, zoo_image

pytestmark = pytest.mark.gpu

TRACE = np.dtype(capi.LightTrace)
DET = np.dtype(capi.Det)


def _as(arr, dt, n):
    return np.frombuffer(arr, dtype=dt)[:n]


def _predict_no_answer(call, L, label_pool):
    """max_contours / points_cap exceeded by the oracle's counts, or the label pool's prefix rule (box order)"""
    out, prefix = [], 0
    for st in call:
        if not st["roi_ok"]:
            out.append(False)
            continue
        need = ls.label_bytes(st["roi"][2], st["roi"][3])
        fits = prefix + need <= label_pool
        prefix += need
        out.append((not fits) or len(st["starts"]) - 1 > L["max_contours"] or len(st["points"]) > L["points_cap"])
    return out


def _check_box(st, T, D, expect_na, L, cov):
    c = st["case"]
    name = (c.group, c.name)
    assert (D["armor_valid"] == -1) == expect_na and bool(T["too_large"]) == expect_na, name
    assert (T["max_contours"], T["points_cap"], T["lds_image"], T["lds_points"]) == (L["max_contours"], L["points_cap"], L["lds_image"], L["lds_points"])
    if not st["roi_ok"]:
        assert T["n_contours"] == 0 and T["n_points"] == 0 and D["armor_valid"] == 0 and D["n_lights"] == 0, name
        return
    assert (T["rx"], T["ry"], T["rw"], T["rh"]) == st["roi"], name
    if not T["pool_fit"]:
        assert expect_na and T["n_contours"] == 0
        return
    assert bool(T["in_lds"]) == (ls.label_bytes(T["rw"], T["rh"]) <= L["lds_image"]), name
    cov["lds_images" if T["in_lds"] else "pool_images"] += 1
    s, p = st["starts"], st["points"]
    n_true = len(s) - 1
    nk = min(n_true, L["max_contours"])
    assert T["n_contours"] == nk and T["n_found"] == min(n_true, L["max_contours"] + 1), (name, T["n_contours"], T["n_found"], n_true)
    assert T["n_points"] == s[nk] and np.array_equal(T["starts"][:nk + 1], s[:nk + 1]), name
    npt = min(int(s[nk]), L["points_cap"])
    assert np.array_equal(T["points"][:npt], p[:npt]), name
    cov["boxes"] += 1
    cov["contours"] += nk
    cov["points"] += npt
    if nk:
        cov["second_chunk_starts"] += int((p[s[:nk], 0] + 1 > 256).sum())
    recs = T["recs"][:nk]
    if expect_na:
        assert not recs["measured"].any() and D["n_lights"] == 0, name
        return
    gated = []
    for i, o in enumerate(st["recs"]):
        r = recs[i]
        assert bool(r["measured"]) == (o is not None), (name, i)
        if o is None:
            continue
        n = s[i + 1] - s[i]
        assert bool(r["in_lds"]) == (n <= L["lds_points"]) and r["hull_edges"] == o.hull_edges, (name, i)
        cov["lds_contours" if r["in_lds"] else "global_contours"] += 1
        cov["hulls_over_64"] += int(o.hull_edges > 64)
        exp = np.array(list(o.corners) + list(o.top) + list(o.bottom) + list(o.center), np.float32)
        got = np.concatenate([r["corners"], r["top"], r["bottom"], r["center"]])
        assert exp.tobytes() == got.tobytes() and np.float64(o.length).tobytes() == r["length"].tobytes() and r["ok"] == o.ok, (name, i, exp, got)
        if o.ok:
            gated.append(r)
    # the final Det: the oracle's, bit for bit, and the trace's last stage
    f = st["final"]
    assert D["armor_valid"] == int(f["ok"]) and D["n_lights"] == f["n_lights"] == len(gated), name
    if f["ok"]:
        assert D["armor_size"] == f["size"] and np.asarray(f["pts"], np.float32).tobytes() == D["kpts"].tobytes(), name
        a, b = gated[-1], gated[-2]
        l, r = (a, b) if a["center"][0] < b["center"][0] else (b, a)
        assert np.concatenate([l["bottom"], l["top"], r["top"], r["bottom"]]).tobytes() == D["kpts"].tobytes(), name
        cov["armors"] += 1
    else:
        assert not D["kpts"].any() and D["pnp_ok"] == 0


def _run_engine(e, rotate, slots):
    L, z = limits(), zoo()
    by_frame = {}
    for st in all_stages():
        by_frame.setdefault(st["case"].frame, []).append(st)
    cov = dict.fromkeys(("boxes", "contours", "points", "lds_images", "pool_images", "lds_contours", "global_contours", "hulls_over_64",
                         "second_chunk_starts", "armors", "no_answer"), 0)
    max_det = e.max_det
    for slot in slots:
        for f, sts in by_frame.items():
            img = zoo_image(f)
            e.get_src_image_buffer(slot)[:] = oracle.rotate180(img) if rotate else img
            for k in range(0, len(sts), max_det):
                call = sts[k:k + max_det]
                boxes = np.array([st["case"].box for st in call], np.float32)
                n = len(call)
                before = bytes(_as(e.extract_armors_raw(boxes, slot), DET, n).tobytes())
                det, trace = e.light_trace(boxes, slot)
                after = bytes(_as(e.extract_armors_raw(boxes, slot), DET, n).tobytes())
                D, T = _as(det, DET, n), _as(trace, TRACE, n)
                assert before == D.tobytes() == after, "a trace call changes nothing extract_armors returns"
                na = _predict_no_answer(call, L, int(T[0]["label_pool"]))
                assert all(x == (st["case"].cap is not None) for x, st in zip(na, call))
                for st, t, d, x in zip(call, T, D, na):
                    _check_box(st, t, d, x, L, cov)
                cov["no_answer"] += sum(na)
                if any(na):      # a box without an answer leaves the others of its call as they are without it
                    keep = [i for i, x in enumerate(na) if not x]
                    alone = _as(e.extract_armors_raw(boxes[keep], slot), DET, len(keep))
                    assert alone.tobytes() == D[keep].tobytes()
    for k, v in cov.items():
        assert v > 0, f"the zoo never reached: {k}"
    return cov


def _engine_test(blob, kind, rotate):
    kw = dict(num_slots=3, rotate180=rotate)
    if kind == "classical":
        kw["point_source"] = capi.POINTS_CLASSICAL
    t0 = time.time()
    with YoloEngine(None, (ls.W, ls.H), weights_blob=blob, **kw) as e:
        assert e._L.irmv_engine_point_source(e._h) == (capi.POINTS_CLASSICAL if kind == "classical" else capi.POINTS_KEYPOINT_HEAD)
        cov = _run_engine(e, rotate, (0, 2))
    print(f"\nlight zoo [{kind} engine, rotate180={int(rotate)}, slots 0 and 2]: " + ", ".join(f"{k} {v}" for k, v in cov.items()) +
          f", worst case none (every stage exact), {time.time() - t0:.1f} s")


@pytest.mark.parametrize("rotate", [True, False])
def test_zoo_on_a_keypoint_engine(blob, rotate):
    _engine_test(blob, "keypoint", rotate)


@pytest.mark.parametrize("rotate", [True, False])
def test_zoo_on_a_classical_engine(blob, rotate):
    _engine_test(blob, "classical", rotate)
