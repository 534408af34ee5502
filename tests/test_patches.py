"""Plate patches on the CPU (include/irmv_hip.h, "plate patches"): the host reference irmv_detection_amd.patches against closed
forms and a brute force, the conditions the GPU tests (tests/test_gpu_patches.py) rest on, and the C ABI's option checks, which
test the values before they look at the engine and so need no GPU."""
import ctypes as C

import numpy as np
import pytest

import patch_set as PS
from irmv_detection_amd import capi, patches as PT


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_identity_patch_is_the_frames_gray():
    """The small plate's quad LT = (40, 30), 31 wide, 12 tall under the default options maps patch pixel (i, j) onto texel
    (46 + i, 23 + j) exactly."""
    f = PS.frame(0)
    p = PT.patch(f, PS.rect_quad((40, 30), 31, 12), 0)
    assert p["state"] == 1 and p["n_outside"] == 0 and p["armor_size"] == 0
    assert np.array_equal(p["gray"], PT.texel_gray(f)[23:51, 46:66].astype(np.uint8))
    assert p["sum"] == int(p["gray"].astype(np.int64).sum())
    # the bars' centre lines are columns 40 and 71, rows 30 .. 42
    assert p["bar_sum"] == (int(f[30:43, [40, 71], 0].astype(np.int64).sum()), int(f[30:43, [40, 71], 2].astype(np.int64).sum()))


def test_corners_map_to_the_keypoints():
    r = np.random.RandomState(5)
    worst = 0.0
    for _ in range(100):
        c = np.array([64.0, 48.0]) + r.uniform(-20, 20, 2)
        w, h = r.uniform(8, 50), r.uniform(4, 24)
        q = np.array([[-w / 2, h / 2], [-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2]]) * r.uniform(0.6, 1.4, (4, 1)) + c + r.uniform(-1, 1, (4, 2))
        k = q.reshape(8).astype(np.float32)
        co = PT.coefficients(k)
        assert co is not None
        x, y, w_ = PT.plate_to_frame(co, [0.0, 0.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0])      # LB, LT, RT, RB
        got = np.stack([x, y], 1).reshape(8)
        worst = max(worst, float(np.abs(got - k.astype(np.float64)).max()))
        assert (w_ > 0).all()
    # a float32 pixel coordinate below 128 has an ulp of 7.6e-6; the fp64 map's own error is some 1e-13 (cancellation in g, h)
    assert worst <= 1e-9, worst


def _otsu_brute(v):
    """Between-class variance in floats at all 256 levels (-1 where a class is empty)."""
    v = np.asarray(v, np.float64).reshape(-1)
    q = np.full(256, -1.0)
    for k in range(256):
        lo, hi = v[v <= k], v[v > k]
        if len(lo) and len(hi):
            q[k] = len(lo) * len(hi) / len(v) ** 2 * (lo.mean() - hi.mean()) ** 2
    return q


def test_otsu_against_a_float_brute_force():
    """200 seeded bimodal patches whose best and second-best between-class variance differ by more than 1e-9 relative (levels
    between which no value lies split the same two classes and have the same q bit for bit: the smallest of them is meant)."""
    r = np.random.RandomState(7)
    done = mismatches = 0
    while done < 200:
        a, b = sorted(r.randint(10, 246, 2))
        n0 = r.randint(100, 460)
        v = np.concatenate([r.normal(a, r.uniform(3, 15), n0), r.normal(b, r.uniform(3, 15), PT.PATCH_N - n0)])
        v = np.clip(np.rint(v), 0, 255).astype(np.int64)
        q = _otsu_brute(v)
        k = int(np.argmax(q))
        rest = q[q != q[k]]
        if not (q[k] - rest.max() > 1e-9 * q[k]):
            continue
        done += 1
        got, S = PT.otsu(v)
        assert S == int(v.sum())
        mismatches += got != k
    assert mismatches == 0
    assert PT.otsu(np.full(PT.PATCH_N, 93)) == (93, 93 * PT.PATCH_N)
    assert PT.otsu(np.zeros(PT.PATCH_N, np.int64)) == (0, 0)


def test_quad_set_keeps_its_distance_from_every_rounding_edge():
    """A condition on the SET: the GPU test demands bytes of every one of these quads, which a floor() one ulp from flipping
    would not allow."""
    k, s = PS.quad_set()
    assert len(k) >= 300 and set(s.tolist()) == {0, 1}
    c = k.reshape(-1, 4, 2).astype(np.float64)
    ctr = c.mean(1)
    assert (np.abs(ctr - np.array(PS.SRC) / 2) <= 21).all()
    m = [PT.rounding_margin(k[i], int(s[i]), None, *PS.SRC) for i in range(len(k))]
    assert min(m) >= PS.MARGIN, min(m)
    ref = PS.quad_set_reference()
    assert all(p["state"] == 1 for p in ref)
    assert len({p["otsu"] for p in ref}) > 20


def test_hard_quads_are_what_they_are_built_for():
    seen = set()
    for name, k, size, opts, fr, state in PS.hard_quads():
        p = PT.patch(PS.hard_frame(fr), k, size, opts)
        if state is not None:
            assert p["state"] == state, (name, p["state"])
        if p["state"] == 0:
            assert not p["gray"].any() and (p["otsu"], p["n_outside"], p["sum"], p["armor_size"]) == (0, 0, 0, 0) and p["bar_sum"] == (0, 0), name
        else:
            assert PT.rounding_margin(k, size, opts, *PS.SRC) >= PS.MARGIN, name
        if "wholly outside" in name or "1e6" in name:
            assert p["n_outside"] == PT.PATCH_N and not p["gray"].any() and p["otsu"] == 0, name
        if "crossing" in name:
            assert 0 < p["n_outside"] < PT.PATCH_N, (name, p["n_outside"])
        if "one-level" in name:
            assert p["otsu"] == fr[1] and (p["gray"] == fr[1]).all(), name
        seen.add(name.split(" ")[0])
    assert {"repeated", "collinear", "nan", "+inf", "-inf", "1e30", "horizon", "wholly", "crossing", "1-pixel", "1e6-pixel", "one-level", "options"} <= seen


def test_reference_refuses_what_the_library_refuses():
    for bad in (dict(span=(18, 54)), dict(span=(33, 54)), dict(span=(32, 130)), dict(light_rows=0), dict(light_rows=29), dict(top=-1), dict(top=28)):
        with pytest.raises(ValueError):
            PT.options(bad)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------
def test_symbols_and_sizes():
    L = capi.load()
    for name in ("irmv_engine_set_patches", "irmv_engine_get_patches", "irmv_engine_plate_patches", "irmv_engine_patches_at", "irmv_patch_limits"):
        assert hasattr(L, name), name
    assert C.sizeof(capi.PlatePatch) == 592 and C.sizeof(capi.PatchOpts) == 32
    assert capi.PlatePatch.state.offset == 560 and capi.PlatePatch.bar_sum.offset == 576 and capi.PlatePatch.sum.offset == 584
    lim = (C.c_int32 * 8)()
    assert L.irmv_patch_limits(lim) == capi.OK
    assert list(lim) == [PT.PATCH_W, PT.PATCH_H, PT.SPAN_MIN, PT.SPAN_MAX, PT.ROWS_MAX, PT.TOP_MAX, 592, 0]
    assert L.irmv_patch_limits(None) == capi.ERR_ARG


def test_option_checks_come_before_the_engine():
    """On a null engine: a refused value answers IRMV_ERR_ARG for the VALUE (the message names it), an accepted one for the
    engine."""
    L = capi.load()

    def call(**kw):
        edit = kw.pop("edit", None)
        o = capi.patch_opts_struct(**kw)
        if edit:
            edit(o)
        rc = L.irmv_engine_set_patches(None, C.byref(o))
        return rc, L.irmv_last_error().decode()

    rc, msg = call()
    assert rc == capi.ERR_ARG and "engine is null" in msg
    for kw in (dict(span=(20, 128)), dict(span=(128, 20)), dict(light_rows=1), dict(light_rows=28), dict(top=0), dict(top=27), dict(enable=0)):
        rc, msg = call(**kw)
        assert rc == capi.ERR_ARG and "engine is null" in msg, (kw, msg)
    bad = [dict(span=(19, 54)), dict(span=(18, 54)), dict(span=(21, 54)), dict(span=(129, 54)), dict(span=(130, 54)),
           dict(span=(32, 19)), dict(span=(32, 18)), dict(span=(32, 55)), dict(span=(32, 130)),
           dict(light_rows=0), dict(light_rows=29), dict(light_rows=-1), dict(top=-1), dict(top=28), dict(enable=2), dict(enable=-1)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == capi.ERR_ARG and "engine is null" not in msg and "patches:" in msg, (kw, msg)

    def res0(o): o.reserved[0] = 1
    def res1(o): o.reserved[1] = -1
    def size(o): o.struct_size = 28
    for edit in (res0, res1, size):
        rc, msg = call(edit=edit)
        assert rc == capi.ERR_ARG and "engine is null" not in msg, msg
    assert L.irmv_engine_set_patches(None, None) == capi.ERR_ARG
    o = capi.PatchOpts()
    assert L.irmv_engine_get_patches(None, C.byref(o)) == capi.ERR_ARG
    n = C.c_int(0)
    assert L.irmv_engine_plate_patches(None, 0, None, 0, C.byref(n)) == capi.ERR_ARG
    assert L.irmv_engine_patches_at(None, 0, None, None, 0, None) == capi.ERR_ARG
    assert L.irmv_engine_patches_at(None, 0, None, None, capi.MAX_DET_CAP + 1, None) == capi.ERR_ARG


# ---- the step fixture --------------------------------------------------------------------------------------------------------
def test_step_fixture_has_survivors(onet):
    """The oracle's CPU step on the step tests' frames at their score threshold: between 8 and max_det survivors, every one of
    which a keypoint engine reports with armor_valid == 1 (nk = 8) -- the GPU step tests cannot pass on an empty list."""
    from oracle import oracle
    for seed in range(3):
        for rot in (True, False):
            head = onet.forward(oracle.preprocess(PS.to_buffer(PS.step_frame(seed), rot), PS.NET[0], rotate180=rot))
            d = oracle.decode_nms(head, PS.NET[0], 14, 8, PS.STEP_THR, 0.45, PS.STEP_MAX_DET)
            assert PS.STEP_MIN <= d["num_dets"] <= PS.STEP_MAX_DET, (seed, rot, d["num_dets"])
            assert d["kpts"].shape == (d["num_dets"], 8) and np.isfinite(d["kpts"]).all()
