"""The input stage's zoo (tests/input_geometry.py) on the CPU: the categories are covered, irmv_front_plan says for every
entry what its label says, the oracle's preprocess stays within its bound of the float64 reference on the whole zoo, the
reference tells the classic wrong variants apart, and irmv_engine_create refuses frames the kernels cannot address."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import input_geometry as ig
import rect_ref
from irmv_detection_amd import _build, bayer, capi
from oracle import oracle


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def plan_of(e):
    return capi.front_plan(e.src, e.net[0], e.net[1], e.mode, e.rot, capi.SRC_HWC8 if e.fmt == "HWC" else e.fmt)


REASONS = {ig.FUSED: capi.FRONT_FUSED, ig.MOD4: capi.FRONT_WIDTH_MOD4, ig.TAP_RANGE: capi.FRONT_TAP_RANGE, ig.STAGE_LIMIT: capi.FRONT_STAGE_LIMIT}


def test_every_category_meets_its_minimum(capsys):
    counts = Counter(c for e in ig.ZOO for c in e.cats)
    with capsys.disabled():
        print(f"\n[input zoo] {len(ig.ZOO)} entries; " + ", ".join(f"{k}: {counts[k]}" for k in ig.MINIMUM))
    short = {k: (counts[k], n) for k, n in ig.MINIMUM.items() if counts[k] < n}
    assert not short, short
    assert set(counts) == set(ig.MINIMUM), set(counts) ^ set(ig.MINIMUM)          # no label without a minimum
    names = {e.name for e in ig.ZOO}
    assert names >= set(ig.REQUIRED_NAMES)
    assert {ig.group_of(e) for e in ig.ZOO} == set(ig.GROUPS)
    for e in ig.ZOO:
        # slots 1 and 2 of every entry whose frames are no multiple of 16 bytes start misaligned
        if e.frame_bytes % 16 or (e.src[0] * e.src[1]) % 16:
            assert e.slots == 3, e.name
        assert e.src[1] <= 1300 or "tall source" in e.cats, e.name
        assert e.net[0] in (64, 96, 128, 160, 256) and e.net[1] in (64, 96, 128, 160, 256), e.name
    assert any(e.net[0] % 64 for e in ig.ZOO if e.expect == ig.FUSED and not e.direct)       # a partial last tile column, staged ...
    assert any(e.net[0] % 64 for e in ig.ZOO if e.expect == ig.FUSED and e.direct)           # ... and direct


def test_labels_say_what_the_geometry_is():
    """The hand-written labels against the letterbox arithmetic, so that a label cannot drift from its entry."""
    for e in ig.ZOO:
        (sw, sh), (W, H) = e.src, e.net
        nw, nh, px, py = ig.letterbox(sw, sh, W, H, e.mode)
        assert nw > 0 and nh > 0, e.name
        c = e.cats
        if "identity" in c: assert (sw, sh) == (nw, nh) == (W, H), e.name
        if "2:1" in c: assert sw == 2 * nw and e.direct, e.name
        if "2:1 rot" in c: assert e.rot and e.direct, e.name
        if "3:1" in c: assert (sw, sh) == (3 * nw, 3 * nh), e.name
        if "4:1" in c: assert (sw, sh) == (4 * nw, 4 * nh), e.name
        if "down" in c: assert 1 < sw / nw < 8 and 1 < sh / nh < 8 and (sw % nw or sh % nh), e.name
        if "mild up" in c: assert 0.55 < sw / nw < 1 and 0.55 < sh / nh < 1, e.name
        if "strong up" in c: assert min(sw, sh) <= 16 and min(sw / nw, sh / nh) <= 0.25, e.name
        for n in (2, 3, 4, 5, 8, 16):
            if f"src {n}" in c: assert n in (sw, sh), e.name
        if "pad x" in c: assert nw < W, e.name
        if "pad y" in c: assert nh < H, e.name
        pads = [W - nw] * ("pad x" in c) + [H - nh] * ("pad y" in c)
        if "pad odd" in c: assert any(p % 2 for p in pads), e.name
        if "pad even" in c: assert any(p and p % 2 == 0 for p in pads), e.name
        if "pad one column" in c: assert px + (W - nw - px) in (1, 2) and W - nw - px == 1, e.name
        if "pad one row" in c: assert H - nh - py == 1, e.name
        if "round .5" in c:
            r = min(W / sw, H / sh)
            assert any(abs(v * r % 1 - 0.5) < 1e-9 for v in (sw, sh)), e.name
        if "narrow box" in c: assert nw < 64 or nh < 16, e.name
        assert e.direct == ("2:1" in c) or sw != 2 * nw, e.name
    pads = {(ig.letterbox(*e.src, *e.net, e.mode)[0] == e.net[0], ig.letterbox(*e.src, *e.net, e.mode)[1] == e.net[1])
            for e in ig.ZOO if e.mode == ig.LETTERBOX}
    assert (False, True) in pads and (True, False) in pads                       # pad in x only, and in y only


def test_plan_matches_category(lib, capsys):
    """irmv_front_plan on every entry: fused or the labelled reason, direct and tall exactly at 2 : 1, the box, the tile
    classes and the pairing cases of the model in tests/input_geometry.py; over the zoo, all four pairing cases and every
    tile class on both paths."""
    cases, classes, fused_with_inside = 0, {"staged": np.zeros(4, int), "direct": np.zeros(4, int)}, 0
    for e in ig.ZOO:
        p, x = plan_of(e), ig.expected_plan(e)                                   # (plan_of raises where the validation rejects)
        assert x["reason"] == e.expect and x["direct"] == e.direct, (e.name, x["reason"], x["direct"])      # the label against the model
        assert p["reason"] == REASONS[e.expect] and p["fused"] == (e.expect == ig.FUSED), (e.name, p)
        assert p["box"] == x["box"], (e.name, p["box"], x["box"])
        assert p["fastx"] == (3 if e.direct else 0), (e.name, p)
        assert p["tile_y"] == x["tile_y"] == (8 if e.direct and p["fused"] else 4), (e.name, p)
        assert (p["tiles_x"], p["tiles_y"]) == x["tiles"], (e.name, p)
        assert (p["fx_i0"], p["fx_step"]) == (x["fx_i0"], x["fx_step"]), (e.name, p)
        assert p["pair_cases"] == sum(ig.PAIR_BITS[c] for c in x["pair_cases"]), (e.name, p, x["pair_cases"])
        got = (p["tiles_inside"], p["tiles_x_edge"], p["tiles_y_edge"], p["tiles_corner"])
        assert got == x["classes"] and sum(got) == p["tiles_x"] * p["tiles_y"], (e.name, got, x["classes"])
        assert p["upload_kernel"] == x["upload_kernel"], (e.name, p)
        assert p["stage_bytes"] >= 4 * p["max_pitch"] * p["max_rows"] or not p["fused"] or e.direct, (e.name, p)
        assert p["stage_bytes"] <= ig.STAGE_MAX or not p["fused"], (e.name, p)
        if p["fused"]:
            cases |= p["pair_cases"]
            classes["direct" if e.direct else "staged"] += got
            # an inside tile and an x-edge tile wherever the geometry can have one: a tile column after the first, and a tile
            # row after the first, whose net-input pixels (64 i - 3 .. 64 (i + 1) - 1, and the same in units of 4 tile_y
            # rows) all lie inside the box
            W, H = e.net
            b, uy = p["box"], 4 * p["tile_y"]
            can = max(1, -(-(b[0] + 3) // 64)) <= min(b[1], W) // 64 - 1 and max(1, -(-(b[2] + 3) // uy)) <= min(b[3], H) // uy - 1
            assert (got[0] >= 1 and got[1] >= 1) == can, (e.name, got, p["box"])
            fused_with_inside += can
    with capsys.disabled():
        print(f"\n[input zoo] tiles inside / x-edge / y-edge / corner: staged {classes['staged'].tolist()}, direct {classes['direct'].tolist()}; "
              f"{fused_with_inside} fused entries have inside tiles; pairing cases 0x{cases:x}")
    assert cases == 0xf
    assert (classes["staged"] > 0).all() and (classes["direct"] > 0).all()
    assert fused_with_inside >= 10


def test_plan_refuses_what_the_engine_refuses(lib):
    for size in ((1, 64), (64, 1), (4097, 64)):
        with pytest.raises(capi.IrmvError):
            capi.front_plan(size, 64)
    with pytest.raises(capi.IrmvError):
        capi.front_plan((64, 64), 80)
    with pytest.raises(capi.IrmvError):
        capi.front_plan((63, 64), 64, src_format="RGGB")
    assert lib.irmv_front_plan(None, None) == capi.ERR_ARG
    # a letterbox whose scaled frame rounds to no row at all (4096 x 2 into 64 x 64: 0.03 rows) has no box and no scale back to
    # the source: refused; one row is enough, and stretching the same frame is fine
    with pytest.raises(capi.IrmvError, match="letterbox"):
        capi.front_plan((4096, 2), 64, resize_mode=capi.RESIZE_LETTERBOX)
    with pytest.raises(capi.IrmvError, match="letterbox"):
        capi.front_plan((2, 1200), 64, 96, resize_mode=capi.RESIZE_LETTERBOX)
    assert capi.front_plan((256, 2), 64, resize_mode=capi.RESIZE_LETTERBOX)["box"] == (0, 64, 31, 32)
    assert capi.front_plan((4096, 2), 64)["box"] == (0, 64, 0, 64)
    # the benchmarked configuration: the 8-row direct tile on every tile
    p = capi.front_plan((1280, 1024), 640)
    assert (p["fused"], p["fastx"], p["tile_y"], p["tiles_x"], p["tiles_y"], p["pair_cases"]) == (True, 3, 8, 10, 20, 4)
    assert (p["fx_i0"], p["fx_step"], p["box"], p["upload_kernel"]) == (1278, -2, (0, 640, 0, 640), True)


def oracle_u8(frame, e):
    """The contract for bit-exactness, as uint8 [h][w][3]: oracle.preprocess on a square net; on a rectangular one its
    numpy restatement tests/rect_ref.py (bit-identical to the oracle on square nets, checked here too)."""
    W, H = e.net
    r = rect_ref.preprocess_u8(frame, W, H, e.mode, e.rot, e.swap)
    if W != H:
        return r
    _, u8 = oracle.preprocess(frame, W, e.mode, e.rot, e.swap, want_u8=True)
    assert np.array_equal(u8, r), e.name
    return u8


def test_oracle_is_anchored_on_the_whole_zoo(capsys):
    """Against the float64 reference, under both figures of test_oracle_preprocess.py::test_matches_float_bilinear_within_one_lsb:
    11-bit coefficients give the rounded float result +-1 LSB, and more than 97 % of an entry's pixels are exactly the
    rounded float result.  On the first frame of every entry; the worst of each is printed."""
    worst, low = (0.0, ""), (1.0, "")
    for e in ig.ZOO:
        for _, frame in ig.slot_frames(e)[:1]:
            u8 = oracle_u8(frame, e)
            ref = ig.reference(frame, e.net, e.mode, e.rot, e.swap)
            err = float(np.abs(u8.astype(np.float64) - ref).max())
            same = float((u8 == np.floor(ref + 0.5)).mean())
            worst, low = max(worst, (err, e.name)), min(low, (same, e.name))
            assert err <= 1.0, (e.name, err)
            assert same > 0.97, (e.name, same)
    with capsys.disabled():
        print(f"\n[input zoo] oracle vs float64: worst |d| {worst[0]:.4f} ({worst[1]}); lowest share of exactly rounded pixels {low[0]:.4f} ({low[1]})")


def _entry(name):
    return next(e for e in ig.ZOO if e.name == name)


@pytest.mark.parametrize("variant,name", [
    ("clamp_early", "up 2x2"),                                   # every tap's partner is the last pixel
    ("clamp_early", "up 8x8"),
    ("corner_aligned", "3:1 64"),
    ("corner_aligned", "up 16x16"),
    ("rotate_after_pad", "pad y odd total rot"),                 # an odd total pad: 25 rows above, 26 below
    ("pad_round_up", "pad y odd total rot"),
    ("pad_round_up", "pad x odd"),
    ("pad_round_up", "one pad column on the right"),
])
def test_wrong_resize_variants_are_seen(variant, name):
    """Each classic wrong variant of the reference moves the named entry by more than the oracle's bound, so the anchor
    test would not pass on it."""
    e = _entry(name)
    frame = ig.slot_frames(e)[0][1]
    ref = ig.reference(frame, e.net, e.mode, e.rot, e.swap)
    bad = ig.reference(frame, e.net, e.mode, e.rot, e.swap, variant=variant)
    assert np.abs(bad - ref).max() > 2.0, (variant, name)
    assert np.abs(oracle_u8(frame, e).astype(np.float64) - bad).max() > 1.0, (variant, name)


def test_right_variants_change_nothing_where_they_cannot():
    """The variants are the reference itself where their mistake cannot show: no rotation, no pad, an even pad."""
    e = _entry("identity 64")
    frame = ig.slot_frames(e)[0][1]
    ref = ig.reference(frame, e.net, e.mode, e.rot, e.swap)
    for v in ("clamp_early", "rotate_after_pad", "pad_round_up", "corner_aligned"):
        assert np.array_equal(ig.reference(frame, e.net, e.mode, e.rot, e.swap, variant=v), ref), v


@pytest.mark.parametrize("border,name", [("reflect", "bayer GRBG 14x6"), ("reflect", "bayer RGGB 2x2"), ("far_clamp", "bayer GBRG 16x8"),
                                         ("far_clamp", "bayer BGGR 30x50")])
def test_wrong_demosaic_borders_are_seen(border, name):
    e = _entry(name)
    raw = ig.slot_frames(e)[0][0]
    good = bayer.demosaic(raw, e.fmt, e.gains)
    assert np.array_equal(ig.demosaic_border(raw, e.fmt, e.gains), good)              # the restatement is the reference
    bad = ig.demosaic_border(raw, e.fmt, e.gains, border)
    d = bad.astype(int) - good
    assert np.abs(d).max() > 0, (border, name)
    H, W = raw.shape
    inner = d[1:H - 1, 1:W - 1]
    assert not inner.size or not inner.any()                                           # only border pixels move
    if border == "far_clamp":
        assert not d[0, :W - 1].any() and not d[:H - 1, 0].any()                      # ... and only at the far border


def test_demosaic_restatement_on_every_bayer_entry():
    for e in ig.ZOO:
        if e.fmt != "HWC":
            for raw, hwc in ig.slot_frames(e):
                assert np.array_equal(ig.demosaic_border(raw, e.fmt, e.gains), hwc), e.name
            if e.gains == ig.SAT_GAINS:
                assert (hwc == 255).any(), e.name


# ---------------------------------------------------------------- frames the kernels cannot address
@pytest.mark.parametrize("size,ok", [
    ((4096, 349525), True),        # 3 * 4096 * 349525 = 2^32 - 12288: the last byte offset fits 32 bits
    ((4096, 349526), False),       # one row more: 2^32 + 0
    ((4095, 349611), False),
    ((2, 2 ** 30), False),
    ((4, 2 ** 31 - 1), False),
])
def test_oversized_frames_are_refused_before_touching_the_gpu(lib, size, ok):
    """k_front.hip's direct tiles hold row * 3 src_width + 3 x as one unsigned 32-bit byte offset: a frame of more than
    2^32 bytes is refused by the validation (irmv_engine_create and irmv_front_plan), before any GPU call."""
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    cfg.src_width, cfg.src_height, cfg.net_size = size[0], size[1], 64
    cfg.weights_path = b"/nonexistent/model.irmw"
    assert (3 * size[0] * size[1] <= capi.MAX_FRAME_BYTES) == ok
    h = C.c_void_p()
    rc = lib.irmv_engine_create(C.byref(cfg), C.byref(h))
    err = lib.irmv_last_error()
    if ok:
        assert rc in (capi.ERR_HIP, capi.ERR_MODEL) and b"too large" not in err, (rc, err)      # accepted until the GPU is needed
    else:
        assert rc == capi.ERR_ARG and b"4294967296" in err and b"src_width * src_height" in err, (rc, err)
    p = capi.FrontPlan()
    assert (lib.irmv_front_plan(C.byref(cfg), C.byref(p)) == capi.OK) == ok
