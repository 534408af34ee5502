"""The refined point source without a GPU: irmv_detection_amd.refine (the bit-exact host reference of the guided ROI, the
cost / admission / choice rule and the flag) against a brute-force restatement, its edge cases, the parameter and creation
checks the library makes before any GPU call, the unchanged ABI struct sizes, the C++ facade, and the oracle-composed
predictions of the scenes tests/test_gpu_refine.py runs (every scene's refined count is confirmed here first)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_craft as rc
from conftest import ROOT
from irmv_detection_amd import _build, capi, refine, weights

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


# ---- select ---------------------------------------------------------------------------------------------------------
def brute_select(lights, kpts, snap):
    """The rule restated on arrays: every light's cost for a side at once, float32 throughout."""
    k = np.asarray(kpts, f32).reshape(4, 2)
    idx = np.array([l[0] for l in lights], np.int64)
    b = np.array([l[1] for l in lights], f32).reshape(-1, 2)
    t = np.array([l[2] for l in lights], f32).reshape(-1, 2)
    s2 = f32(snap) * f32(snap)
    pick = []
    for B, T in ((k[0], k[1]), (k[3], k[2])):
        db, dt = b - B, t - T
        cost = (db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + (dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1])
        d = B - T
        thr = s2 * (d[0] * d[0] + d[1] * d[1])
        adm = np.nonzero(cost <= thr)[0]
        if len(adm) == 0:
            pick.append(None)
            continue
        best = cost[adm].min()
        pick.append(int(idx[adm[cost[adm] == best]].max()))
    return (pick[0] is not None and pick[1] is not None and pick[0] != pick[1]), pick[0], pick[1]


def test_select_against_brute_force():
    rng = np.random.default_rng(7)
    seen = {"refined": 0, "none": 0, "same": 0}
    for trial in range(400):
        c = rng.uniform(40, 200, 2)
        k = (c + rc.QUAD.astype(np.float64) + rng.normal(0, 1.5, (4, 2))).astype(f32).reshape(8)
        n = int(rng.integers(0, 7))
        lights = []
        for i in rng.permutation(n):
            x = c[0] + rng.choice([-20, 20, 0]) + rng.normal(0, 4)
            y0 = c[1] - 12 + rng.normal(0, 4)
            lights.append((int(i), (f32(x), f32(y0 + 24)), (f32(x + rng.normal(0, 1)), f32(y0))))
        snap = float(rng.choice([0.1, 0.25, 0.5, 1.0, 4.0]))
        got, ref = refine.select(lights, k, snap), brute_select(lights, k, snap) if n else (False, None, None)
        assert got == ref, (trial, got, ref)
        seen["refined"] += got[0]
        seen["none"] += got[1] is None or got[2] is None
        seen["same"] += got[1] is not None and got[1] == got[2]
    assert min(seen.values()) >= 5, seen


def test_tie_goes_to_the_later_contour():
    """Mirrored integer-coordinate bars: both lights cost exactly the same in fp32, the higher contour index wins -- whatever
    the order they are handed over in."""
    k = np.array([50, 80, 50, 40, 90, 40, 90, 80], f32)       # LB, LT, RT, RB
    a = (3, (f32(47), f32(81)), (f32(47), f32(41)))           # 3 px left of side L, 1 px down
    b = (9, (f32(53), f32(81)), (f32(53), f32(41)))           # its mirror image about x = 50
    r = (5, (f32(90), f32(80)), (f32(90), f32(40)))
    B, T = refine.sides(k)[0]
    assert refine.cost(a[1], a[2], B, T) == refine.cost(b[1], b[2], B, T) == f32(20)
    for order in ([a, b, r], [b, a, r], [r, b, a]):
        assert refine.select(order, k, 0.5) == (True, 9, 5)
    assert refine.select([(9,) + a[1:], (3,) + b[1:], r], k, 0.5) == (True, 9, 5)
    assert refine.select([a, r], k, 0.5) == (True, 3, 5)


def test_one_light_for_both_sides_is_not_refined():
    k = np.array([50, 80, 50, 40, 90, 40, 90, 80], f32)
    mid = (0, (f32(70), f32(80)), (f32(70), f32(40)))
    assert refine.select([mid], k, 0.25) == (False, None, None)        # 2 * 400 > 0.0625 * 1600
    assert refine.select([mid], k, 1.0) == (False, 0, 0)               # admissible for both: one contour, no pair
    far = (1, (f32(91), f32(80)), (f32(91), f32(40)))
    assert refine.select([mid, far], k, 1.0) == (True, 0, 1)


def test_zero_length_side_admits_only_an_exact_hit():
    k = np.array([50, 60, 50, 60, 90, 40, 90, 80], f32)                # LB == LT: len2 = 0
    near = (0, (f32(50), f32(61)), (f32(50), f32(60)))
    hit = (1, (f32(50), f32(60)), (f32(50), f32(60)))
    r = (2, (f32(90), f32(80)), (f32(90), f32(40)))
    assert refine.select([near, r], k, 4.0) == (False, None, 2)
    assert refine.select([hit, near, r], k, 4.0) == (True, 1, 2)       # cost 0 <= 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 24, -(2.0 ** 24), 1e30])
def test_unusable_keypoints(bad):
    k = np.array([50, 80, 50, 40, 90, 40, 90, 80], f32)
    lights = [(0, (f32(50), f32(80)), (f32(50), f32(40))), (1, (f32(90), f32(80)), (f32(90), f32(40)))]
    assert refine.select(lights, k, 0.5) == (True, 0, 1)
    for i in range(8):
        d = k.copy()
        d[i] = bad
        assert not refine.usable(d) and refine.guided_box([40, 30, 100, 90], d, 4.0) is None
        assert refine.select(lights, d, 0.5) == (False, None, None)
    edge = k.copy()
    edge[3] = np.nextafter(f32(2.0 ** 24), f32(0))
    assert refine.usable(edge) and refine.guided_box([40, 30, 100, 90], edge, 4.0) is not None
    assert refine.flag(False, True) == 1 and refine.flag(False, True, pnp_ok=False) == 0 and refine.flag(False, False) == 0
    assert refine.flag(True, False) == -1 and refine.flag(True, True) == -1


def test_guided_box_and_its_roi():
    from oracle import oracle
    k = np.array([50, 80, 50, 40, 90, 40, 90, 80], f32)
    assert refine.guided_box([60, 50, 80, 70], k, 4.0).tolist() == [46, 36, 94, 84]             # the keypoints' hull + margin
    assert refine.guided_box([40, 30, 100, 90], k, 0.0).tolist() == [40, 30, 100, 90]           # the box's own
    assert refine.guided_box([40.5, 30.25, 100, 90], k, 0.5).tolist() == [40, 29.75, 100.5, 90.5]
    # negative coordinates and beyond the frame: the box keeps them, the classical ROI rule clamps and truncates
    neg = np.array([-7.5, 100, -7.5, 60, 30, 60, 30, 100], f32)
    g = refine.guided_box([-3, 55, 20, 140], neg, 4.0)
    assert g.tolist() == [-11.5, 51, 34, 144]
    assert oracle.light_roi(256, 128, g)[:2] == (True, (0, 51, 34, 77))
    out = np.array([250, 120, 250, 100, 300.5, 100, 300.5, 120], f32)
    g = refine.guided_box([240, 90, 256, 128], out, 4.0)
    assert g.tolist() == [236, 86, 304.5, 132]
    assert oracle.light_roi(256, 128, g)[:2] == (True, (236, 86, 20, 42))
    gone = np.array([300, 120, 300, 100, 340, 100, 340, 120], f32)
    assert not oracle.light_roi(256, 128, refine.guided_box([290, 90, 350, 128], gone, 4.0))[0]   # wholly outside: no ROI
    assert refine.label_bytes(256, 128) == 33552 and refine.label_bytes(1, 1) == 16


# ---- what the library checks before any GPU call -------------------------------------------------------------------------
@pytest.mark.parametrize("snap,margin,word", [(0.0, 4.0, b"snap"), (-1.0, 4.0, b"snap"), (4.0001, 4.0, b"snap"), (np.nan, 4.0, b"snap"),
                                              (0.5, -0.001, b"roi_margin"), (0.5, 64.5, b"roi_margin"), (0.5, np.nan, b"roi_margin"),
                                              (np.inf, 4.0, b"snap"), (0.5, np.inf, b"roi_margin")])
def test_refused_parameters(lib, snap, margin, word):
    """The values are judged before the engine is looked at: a refused one never reaches it."""
    assert lib.irmv_engine_set_refine(None, snap, margin) == capi.ERR_ARG
    assert word in lib.irmv_last_error()
    with pytest.raises(ValueError):
        refine.check_params(snap, margin)


def test_accepted_parameters_reach_the_engine_check(lib):
    for snap, margin in ((0.5, 4.0), (4.0, 0.0), (1e-3, 64.0)):
        refine.check_params(snap, margin)
        assert lib.irmv_engine_set_refine(None, snap, margin) == capi.ERR_ARG and b"engine is null" in lib.irmv_last_error()
    assert lib.irmv_engine_get_refine(None, None, None) == capi.ERR_ARG
    assert (refine.DEFAULT_SNAP, refine.DEFAULT_ROI_MARGIN) == (0.5, 4.0)


def _create(lib, blob, point_source):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    keep = C.create_string_buffer(blob, len(blob))
    cfg.weights_blob, cfg.weights_bytes = C.cast(keep, C.c_void_p), len(blob)
    cfg.point_source = point_source
    h = C.c_void_p()
    rc_ = lib.irmv_engine_create(C.byref(cfg), C.byref(h))
    return rc_, lib.irmv_last_error(), h


def test_refined_needs_a_keypoint_head(lib, blob, tmp_path):
    """A model without a keypoint head is refused with the model error before any GPU call -- from memory and from a file;
    with a keypoint head the same call gets as far as the device check (here: no device)."""
    import torch
    bbox_only = weights.synthetic_blob(0, nk=0)
    code, msg, _ = _create(lib, bbox_only, capi.POINTS_REFINED)
    assert code == capi.ERR_MODEL and b"keypoint head" in msg
    path = tmp_path / "m.irmw"
    path.write_bytes(bbox_only)
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    cfg.weights_path = os.fsencode(str(tmp_path / "m.onnx"))
    cfg.point_source = capi.POINTS_REFINED
    h = C.c_void_p()
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_MODEL and b"keypoint head" in lib.irmv_last_error()
    cfg.point_source = 4
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG and b"point_source" in lib.irmv_last_error()
    if not torch.cuda.is_available():
        assert _create(lib, blob, capi.POINTS_REFINED)[0] == capi.ERR_HIP
    assert capi.POINTS_REFINED == 3


def test_abi_sizes_unchanged(tmp_path):
    """irmv_det and irmv_engine_cfg keep the sizes they had before the refined source (the flag lives in `reserved`)."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu %d\\n", sizeof(irmv_det),'
                   ' sizeof(irmv_engine_cfg), offsetof(irmv_det, reserved), IRMV_POINTS_REFINED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"160", b"280", b"156", b"3"]
    assert (C.sizeof(capi.Det), C.sizeof(capi.EngineCfg), capi.Det.reserved.offset) == (160, 280, 156)


# ---- C++ facade -------------------------------------------------------------------------------------------------------
def facade_exe(build=True):
    """tests/cpp/refine_facade_test.cpp against the facade headers (built here so that the binary travels to the GPU box with the tree)."""
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    exe = os.path.join(bindir, "refine_facade_test")
    if build or not os.path.exists(exe):
        os.makedirs(bindir, exist_ok=True)
        _build.build()
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "refine_facade_test.cpp"), "-o", exe,
                               "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_facade_compiles_with_the_point_source_argument():
    exe = facade_exe()
    assert subprocess.call([exe]) == 2          # without arguments: the core's parameters only, no engine


# ---- the GPU tests' scenes, predicted here first -------------------------------------------------------------------------
def test_step_scene_prediction():
    """The eight-plate frame of the whole-step cases: the oracle-composed prediction gives the refined count the scene is
    built for, the refined points are the drawn bars' ends, and the decoy bar of plate 4 does not change the pair."""
    img, want = rc.step_scene()
    boxes, kpts = rc.step_detections()
    pred = rc.predict(img, boxes, kpts)
    assert [p["flag"] for p in pred] == want and sum(want) == 4
    assert [p["n_lights"] for p in pred] == [2, 2, 1, 2, 3, 2, 0, 1]
    c = rc.plate_centres()[0]
    ends = rc.plate_bars(rc.blank(), c, left=(-1, 1), right=(1, -2))
    assert pred[0]["kpts"].tolist() == [float(v) for p in ends for v in p]
    assert pred[0]["kpts"].tolist() == [10.5, 44, 10.5, 21, 53.5, 18, 53.5, 41]
    for p, k in zip(pred, kpts):
        assert (p["flag"] == 1) != np.array_equal(p["kpts"], k)
        if p["flag"] == 1:
            assert 1.0 <= np.abs(p["kpts"] - k).max() <= 3.0          # the keypoints were 1 - 3 px off the bars
    # with everything admissible (snap 4) plate 2's one bar serves both sides, plate 3's cut bars are taken
    wide = rc.predict(img, boxes, kpts, snap=4.0)
    assert [p["flag"] for p in wide] == [1, 1, 0, 1, 1, 1, 0, 0] and refine.select(wide[2]["lights"], kpts[2], 4.0) == (False, 0, 0)
    # the same scene inside the full frame at the window tests' bottom-right corner
    org = (rc.FULL[0] - rc.WIN[0], rc.FULL[1] - rc.WIN[1])
    big, _ = rc.step_scene(rc.FULL, org)
    b2, k2 = rc.step_detections(org)
    assert [p["flag"] for p in rc.predict(big, b2, k2)] == want
    assert np.array_equal(big[org[1]:, org[0]:], img)
