"""The references at class counts other than 14 (tests/class_counts.py), before they judge the GPU
(tests/test_gpu_class_counts.py).  No GPU.

  * oracle.decode_nms at every nc of NCS against a brute-force numpy walk over ids // nc and ids % nc;
  * detect_craft.closed_form equals the oracle bit for bit on the `edge` and `all` class biases, at 64 x 64 and 96 x 96, for
    every (nc, nk) pair;
  * DENSITY: seeded random heads of 8400 anchors per nc whose candidate counts sit in the post stage's tiers (up to 512, up
    to 1024, up to 8192, more than the key list's sort holds);
  * NATURAL: per nc a shift of the class finals that leaves 1 .. A nc / 2 candidates on the 96 x 96 (and the 64 x 64) net,
    also when the threshold moves by HEAD_TOL either way;
  * class_policy.table against irmv_class_policy_table (host code of the library) for a policy with class nc - 1 off and one
    with only class nc - 1 on.
"""
import numpy as np
import pytest

import class_counts as cc
import detect_craft as dc
from irmv_detection_amd import _build, capi, class_policy, frames
from oracle import oracle
from test_detect_craft import HEAD_TOL
from test_oracle_post import np_iou

NCS, PAIRS = cc.NCS, cc.PAIRS

# nc -> {T: (seed, the oracle's n_candidates)}: cc.density_head(nc, nk, T, seed) at 8400 anchors, nk = 8 (the class columns
# are drawn before the keypoint columns: nk = 0 gives the same classes, so the same count).  Tiers: T = 300 -> 1 .. 512,
# 770 -> 513 .. 1024, 3000 -> 1025 .. 8192 (each with a fifth of the band clear of either edge), 20000 -> more than 10000.
# nc = 1 has 8400 pairs: no 20000.
DENSITY = {
    1: {300: (100, 284), 770: (101, 779), 3000: (102, 3005)},
    4: {300: (400, 318), 770: (401, 717), 3000: (402, 2976), 20000: (403, 19961)},
    5: {300: (500, 293), 770: (501, 785), 3000: (502, 3011), 20000: (503, 20076)},
    13: {300: (1300, 272), 770: (1301, 703), 3000: (1302, 2919), 20000: (1303, 20145)},
    16: {300: (1600, 310), 770: (1601, 771), 3000: (1602, 3029), 20000: (1603, 19967)},
}
TIERS = {300: (1, 512), 770: (513, 1024), 3000: (1025, 8192)}

# nc -> (delta, {net: (the oracle's n_candidates on frames 3, 4, 5, the counts with the threshold HEAD_TOL higher .. lower)}): the
# class finals of cc.blob(nc) shifted by delta, on the 96 x 96 net (A = 189) and, for the GPU module's 64x3 engine, on the
# 64 x 64 net (A = 84).  The band is 1 .. A nc / 2.
NATURAL_FRAMES = (3, 4, 5)
NATURAL = {
    1: (5.0, {96: ((43, 44, 41), ((36, 44), (37, 45), (40, 43))), 64: ((17, 17, 17), ((15, 20), (12, 19), (14, 19)))}),
    4: (5.0, {96: ((147, 149, 147), ((142, 160), (137, 158), (137, 158))), 64: ((65, 65, 65), ((64, 73), (63, 77), (63, 70)))}),
    5: (5.0, {96: ((185, 180, 172), ((172, 202), (166, 187), (163, 183))), 64: ((85, 81, 82), ((76, 94), (77, 93), (73, 92)))}),
    13: (5.0, {96: ((465, 464, 456), ((441, 477), (440, 478), (432, 478))), 64: ((211, 209, 211), ((200, 214), (201, 214), (203, 213)))}),
    16: (5.0, {96: ((610, 605, 597), ((568, 641), (559, 635), (558, 623))), 64: ((267, 271, 268), ((252, 287), (256, 288), (251, 284)))}),
}


def natural_band(A, nc):
    return 1, (A * nc) // 2


# ---- b. the oracle against brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", NCS)
def test_oracle_matches_bruteforce_walk(nc):
    W, nk = 160, 8                                                  # 400 + 100 + 25 anchors
    A = sum(dc.level_sizes(W, W))
    rng = np.random.default_rng(20 + nc)
    for hot, thr, iou_thr, max_det in ((0.3 / nc, 0.25, 0.45, 100), (0.6 / nc, 0.4, 0.6, 30), (0.02 / nc, 0.25, 0.45, 100)):
        head = cc.random_head(rng, A, nc, nk, hot)
        assert head.shape == (A, 64 + nc + nk)
        d = oracle.decode_nms(head, W, nc, nk, thr, iou_thr, max_det)
        boxes, keys = oracle.decode_candidates(head, W, nc, nk, thr)
        cls_logits = head[:, 64:64 + nc]
        n = int((cls_logits > dc.logit_thr(thr)).sum())
        assert d["n_candidates"] == len(keys) == n > 0
        ids = (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
        assert ids.max() < A * nc
        anc, cls = ids // nc, ids % nc
        logits = cls_logits[anc, cls]
        assert (np.diff(logits) <= 0).all() and (np.diff(ids)[np.diff(logits) == 0] > 0).all()
        keep = []
        for i in range(len(ids)):
            if len(keep) >= max_det:
                break
            if all(not (cls[j] == cls[i] and np_iou(boxes[anc[j]].astype(np.float64), boxes[anc[i]].astype(np.float64)) > iou_thr) for j in keep):
                keep.append(i)
        assert d["num_dets"] == len(keep) > 0
        assert list(d["anchors"]) == list(anc[keep]) and list(d["classes"]) == list(cls[keep])
        assert d["classes"].max() < nc and d["kpts"].shape == (len(keep), nk)
        logit = head[d["anchors"], 64 + d["classes"]].astype(np.float64)
        assert np.abs(d["scores"] - 1 / (1 + np.exp(-logit))).max() < 1e-6


def test_random_head_is_the_recipe_of_test_oracle_post():
    from test_oracle_post import _random_head
    a = _random_head(np.random.default_rng(9), 500, 14, 8, 0.01)
    b = cc.random_head(np.random.default_rng(9), 500, 14, 8, 0.01)
    assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- c, d. bias vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", NCS)
def test_bias_vectors(nc):
    thr = dc.logit_thr(0.25)
    e = cc.edge_bias(nc)
    assert e.shape == (nc,) and e.dtype == np.float32
    assert list(np.nonzero(e > thr)[0]) == [nc - 1]
    assert e[nc - 1].view(np.int32) == thr.view(np.int32) - 1            # negative floats: one ulp up is one bit pattern down
    if nc >= 2:
        assert e[0] == thr
    if nc >= 3:
        assert e[nc - 2].view(np.int32) == thr.view(np.int32) + 1
        assert (np.delete(e, [0, nc - 2, nc - 1]) == dc.DARK).all()
    a = cc.all_lit_bias(nc)
    assert a.shape == (nc,) and (a == np.float32(1.25)).all()


# ---- e. closed form against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 96])
@pytest.mark.parametrize("pair", PAIRS, ids=cc.pair_id)
def test_closed_forms_equal_the_oracle(pair, W):
    nc, nk = pair
    kp = dc.quad_kpt_bias(nk)
    A = sum(dc.level_sizes(W, W))
    for name, bias, md in (("edge", cc.edge_bias(nc), 100), ("all", cc.all_lit_bias(nc), 256)):
        head = dc.expected_head(W, W, bias, dc.POINT_BOXES, kp)
        assert head.shape == (A, 64 + nc + nk)
        cf = dc.closed_form(W, W, bias, 0, kp, 0.25, md, 4096)
        exp = oracle.decode_nms(head, W, nc, nk, max_det=md)
        want = A if name == "edge" else A * nc
        assert cf["n_candidates"] == exp["n_candidates"] == want
        assert cf["num_dets"] == exp["num_dets"] == min(md, want)
        for k in ("anchors", "classes", "boxes", "kpts"):
            assert cf[k].shape == exp[k].shape and np.array_equal(cf[k], exp[k]), (name, k)
        if name == "edge":
            assert (cf["order_classes"] == nc - 1).all() and np.array_equal(cf["order_anchors"], np.arange(A))
        else:       # ordered by anchor, then by class
            assert np.array_equal(cf["order_anchors"], np.repeat(np.arange(A), nc))
            assert np.array_equal(cf["order_classes"], np.tile(np.arange(nc), A))


# ---- f. density table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", NCS)
def test_density_table_sits_inside_its_tiers(nc, capsys):
    assert tuple(DENSITY[nc]) == cc.density_ts(nc) and (20000 in DENSITY[nc]) == (nc > 1)
    lines = []
    for T, (seed, want) in DENSITY[nc].items():
        head = cc.density_head(nc, 8, T, seed)
        d = oracle.decode_nms(head, 640, nc, 8)
        n = d["n_candidates"]
        lines.append(f"  nc {nc} T {T} seed {seed}: oracle {n} candidates, {d['num_dets']} survivors")
        assert n == int((head[:, 64:64 + nc] > dc.logit_thr(0.25)).sum()) == want
        if T in TIERS:
            assert dc.inside_with_margin(n, *TIERS[T]), (nc, T, n)
        else:
            assert n > 10000
        assert 0 < d["num_dets"]
        if nc in (1, 16):       # without keypoints: the same class columns, so the same count
            h0 = cc.density_head(nc, 0, T, seed)
            assert np.array_equal(h0[:, :64 + nc], head[:, :64 + nc])
            assert oracle.decode_nms(h0, 640, nc, 0)["n_candidates"] == n
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- g. natural-weights shift ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [96, 64])
@pytest.mark.parametrize("nc", NCS)
def test_natural_shift_sits_inside_its_band(nc, W, capsys):
    A = sum(dc.level_sizes(W, W))
    delta, per_net = NATURAL[nc]
    counts, brackets = per_net[W]
    lo, hi = natural_band(A, nc)
    net = oracle.Net(dc.craft(cc.blob(nc), cls=("shift", delta)))
    thr = dc.logit_thr(0.25)
    inside, lines = 0, []
    for f, want, (w_hi, w_lo) in zip(NATURAL_FRAMES, counts, brackets):
        head = net.forward(oracle.preprocess(frames.synthetic_frame(f), W))
        assert head.shape == (A, 64 + nc + 8)
        cl = head[:, 64:64 + nc]
        n = oracle.decode_nms(head, W, nc, 8)["n_candidates"]
        n_hi, n_lo = int((cl > thr + HEAD_TOL).sum()), int((cl > thr - HEAD_TOL).sum())
        lines.append(f"  nc {nc} net {W} delta {delta:+g} frame {f}: oracle {n} candidates (threshold +/- HEAD_TOL: {n_hi} .. {n_lo}), band {lo} .. {hi}")
        assert n == int((cl > thr).sum()) == want and (n_hi, n_lo) == (w_hi, w_lo)
        inside += lo <= n_hi <= n <= n_lo <= hi
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert inside >= 2


# ---- h. class policy table -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


@pytest.mark.parametrize("nc", NCS)
def test_policy_tables_match_the_library(lib, nc):
    for name, p in (("last off", cc.last_off_policy(nc)), ("only last", cc.only_last_policy(nc))):
        thr, mn = capi.class_policy_table(capi.class_policy_struct(p["score_thr"], p["plate"]), nc)
        thr = np.asarray(thr, np.float32)
        ref, ref_mn = class_policy.table(p, nc)
        assert np.array_equal(thr.view(np.uint32), ref.view(np.uint32)), (name, thr, ref)
        assert np.float32(mn).view(np.uint32) == np.float32(ref_mn).view(np.uint32), (name, mn, ref_mn)
        assert np.isposinf(thr[nc:]).all()                            # at and above nc: +inf, whatever the policy holds there
        on = [nc - 1] if name == "only last" else list(range(nc - 1))
        assert list(np.nonzero(np.isfinite(thr))[0]) == on
        if on:                                                        # the minimum is taken over c < nc only
            assert mn == thr[:nc].min() == thr[on[0]] and np.isfinite(mn)
            assert mn == dc.logit_thr(p["score_thr"][on[0]])
            if nc < 16:
                assert mn > dc.logit_thr(p["score_thr"][nc:].min())  # ... the entries behind nc hold a smaller threshold
        else:
            assert nc == 1 and np.isposinf(mn) and class_policy.min_score_thr(p, nc) is None
