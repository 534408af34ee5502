"""The engine at class counts other than 14: nc = 1, 4, 5, 13, 16 (tests/class_counts.py says why these), nk = 8, and nk = 0 at
nc 1 and 16.  The references are proven at these counts on the CPU first (tests/test_class_counts.py).

  1. The post stage alone (write_head + run_post: scan_decode_kernel and nms_pnp_kernel) on a 640 x 640 engine per (nc, nk):
     the first head an engine sees is the empty one (all nc classes at -20, the record's class slots nc .. 15 still the 0.0
     of the allocation: a scanner without its `class < nc` mask finds a score of 0.5 there); the density heads of
     test_class_counts.DENSITY (a head per NMS tier); every pair lit and tied (A nc candidates: the key list's capacity);
     tied runs on the first and the last class.  Every field of read_raw against oracle.decode_nms, bit for bit, on the default
     caps and on (pre_nms_cap, max_det) = (150, 100) and (2048, 256) -- and once more under IRMV_POST_KEYS_ONLY=1, the
     class-major path every whole step takes, with IRMV_NMS_CLASSWALK 1 and 0.
  2. Whole steps on crafted finals through test_gpu_detect_craft.check_step on the 64x3 (single-frame shares, grouped Detect
     launches) and 96x3 (one batched share) engines, untuned: `edge` (class nc - 1 one ulp above the threshold, class 0 on it,
     class nc - 2 one ulp below: A candidates), `all` (A nc candidates), `wide` (all lit, wide boxes: chains in every class),
     `natural` (the class finals shifted by test_class_counts.NATURAL's delta; nk = 8 only, the table's blobs); `edge` and
     `all` again through the other two producers and the dense head; results() at nc = 16 reports classes 14 and 15 as 14.
  3. The layers: test_gpu_conv_candidates.sweep at nc 1, 5, 16 (every tile candidate of every conv op, the class finals with
     cout = nc in a 16-row pad among them, bitwise against the step and against the fp64 reference under the existing
     bound), and the head against the fp32 oracle under HEAD_TOL.
  4. The class policy: class nc - 1 off (A (nc - 1) candidates; none at nc = 1) and only class nc - 1 on (A), through
     test_gpu_class_policy.check_policy_step, and run_post on random heads under the first policy.

Every case passed on the first run: no defect of the engine showed at these class counts.  The `class < nc` mask of a producer
is not the only guard in front of a padded class -- the policy table's +inf entries at and above nc fail the per-class test of
all three producers, and the two scanners of k_post.hip test `c < a.nc` once more at the key store --, so the cases here hold
these guards together: a padded class reaches the key list only where all of them fail.

Wall time of the module on an MI355X: 127 tests, 28 s together, the slowest 0.6 s.
"""
import contextlib
import functools
import time

import numpy as np
import pytest

import class_counts as cc
import detect_craft as dc
from irmv_detection_amd import class_policy as cp, frames
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_class_counts import DENSITY, NATURAL, NATURAL_FRAMES, natural_band
from test_gpu_class_policy import check_policy_step, engine as policy_engine, reference, run as run_policy, same_raw
from test_gpu_conv_candidates import _report, conv_ops, layer_table, load_frames, sweep
from test_gpu_detect_craft import ENGINES, SRC, SWITCHES, check_step, decode, engine, env, run_case
from test_gpu_engine import HEAD_TOL, _raw_tuple

pytestmark = pytest.mark.gpu

NCS, PAIRS, A640 = cc.NCS, cc.PAIRS, cc.A640
CAPS = [(4096, 100), (150, 100), (2048, 256)]       # (pre_nms_cap, max_det): the default, a cap below most counts, the largest max_det


# ---- 1. the post stage alone ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def post_heads(nc, nk):
    """name -> (head, n_candidates known beforehand or None); the empty head first."""
    out = {"empty": (cc.empty_head(nc, nk), 0)}
    for T, (seed, n) in DENSITY[nc].items():
        out[f"density {T}"] = (cc.density_head(nc, nk, T, seed), n)
    out["all pairs"] = (cc.all_pairs_head(nc, nk), A640 * nc)
    ties = cc.tie_heads(nc, nk)
    out["first and last class"] = (ties["first and last class"], 601 if nc > 1 else 301)
    out["two classes per anchor"] = (ties["two classes per anchor"], 400 if 4 % nc != 9 % nc else 300)
    return out


@functools.lru_cache(maxsize=None)
def post_expected(nc, nk, cap, md, name):
    return oracle.decode_nms(post_heads(nc, nk)[name][0], 640, nc, nk, max_det=md, pre_nms_cap=cap)


@contextlib.contextmanager
def post_engine(nc, nk, cap, md, keys_only=None, classwalk=None):
    """640 x 640, one slot, untuned: only the post kernels ever run on it."""
    pins = dict(IRMV_AUTOTUNE="0", IRMV_POST_KEYS_ONLY=keys_only, IRMV_NMS_CLASSWALK=classwalk, **{k: None for k in SWITCHES})
    with env(**pins):
        e = YoloEngine(None, SRC, weights_blob=cc.blob(nc, nk), num_slots=1, pre_nms_cap=cap, max_det=md)
    try:
        assert e.num_anchors == A640 and e.head_channels == 64 + nc + nk
        yield e
    finally:
        e.close()


def post_exact(e, nc, nk, cap, md, name, lines):
    """test_gpu_engine._assert_post_exact with nc and nk passed through."""
    head, known = post_heads(nc, nk)[name]
    exp = post_expected(nc, nk, cap, md, name)
    e.write_head(head, 0)
    e.run_post(0, 1)
    raw = e.read_raw(0)
    lines.append(f"  {name}: n_candidates {raw['n_candidates']} (oracle {exp['n_candidates']}), num_dets {raw['num_dets']} (oracle {exp['num_dets']})")
    assert exp["n_candidates"] == known, (name, exp["n_candidates"], known)
    same_raw(raw, exp, nk, name)
    assert (raw["classes"] < nc).all() and not raw["kpts"][:, nk:].any(), name
    return raw


def run_post_heads(capsys, tag, nc, nk, cap, md, **kw):
    t0, lines, got = time.time(), [], {}
    try:
        with post_engine(nc, nk, cap, md, **kw) as e:
            for name in post_heads(nc, nk):              # "empty" first: nothing has written the record's class slots nc .. 15
                raw = post_exact(e, nc, nk, cap, md, name, lines)
                got[name] = _raw_tuple(raw)
                if name == "empty":
                    assert raw["n_candidates"] == 0 and raw["num_dets"] == 0
                if name == "all pairs":
                    assert raw["n_candidates"] == A640 * nc and raw["num_dets"] > 0
    finally:
        with capsys.disabled():
            print(f"\n[class counts, post alone: {tag}] {time.time() - t0:.1f} s\n" + "\n".join(lines))
    return got


POST_CASES = [(p, c) for p in PAIRS for c in CAPS]
POST_IDS = [f"{cc.pair_id(p)}-cap{c[0]}-md{c[1]}" for p, c in POST_CASES]


@pytest.mark.parametrize("pair,caps", POST_CASES, ids=POST_IDS)
def test_post_alone(capsys, pair, caps):
    (nc, nk), (cap, md) = pair, caps
    assert set(DENSITY[nc]) == set(cc.density_ts(nc))
    run_post_heads(capsys, f"nc {nc} nk {nk} cap {cap} max_det {md}", nc, nk, cap, md)


@pytest.mark.parametrize("pair,caps", POST_CASES, ids=POST_IDS)
def test_post_class_major_path(capsys, pair, caps):
    """IRMV_POST_KEYS_ONLY=1: run_post's NMS decodes its own boxes, as a whole step's does -- the class-major walk (nc ballots, the
    16-lane prefix sum over lane < nc, one walking wave per class) and, with IRMV_NMS_CLASSWALK=0, the older walk."""
    (nc, nk), (cap, md) = pair, caps
    got = {cw: run_post_heads(capsys, f"nc {nc} nk {nk} cap {cap} max_det {md} keys only, class walk {cw}", nc, nk, cap, md, keys_only="1", classwalk=cw)
           for cw in ("1", "0")}
    for name in post_heads(nc, nk):
        a, b = got["1"][name], got["0"][name]
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), name


# ---- 2. whole steps on crafted finals ---------------------------------------------------------------------------------------
def crafted(nc, nk, case, W, H):
    """-> (blob, check_step keywords) of a case."""
    kp = dc.quad_kpt_bias(nk)
    base = cc.blob(nc, nk)
    kw = dict(nc=nc, nk=nk)
    if case == "edge":
        bias = cc.edge_bias(nc)
        b = dc.craft(base, cls=("bias", bias), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
        kw.update(closed=dc.closed_form(W, H, bias, 0, kp, 0.25, 100, 4096))
    elif case == "all":
        bias = cc.all_lit_bias(nc)
        b = dc.craft(base, cls=("bias", bias), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
        kw.update(max_det=256, closed=dc.closed_form(W, H, bias, 0, kp, 0.25, 256, 4096))
    elif case == "wide":
        bias = cc.all_lit_bias(nc)
        b = dc.craft(base, cls=("bias", bias), box=("bias", dc.WIDE_BOXES), kpt=("bias", kp))
        kw.update(closed=dc.closed_form(W, H, bias, 15, kp))
    elif case == "natural":
        assert nk == 8                      # NATURAL is the table of the nk = 8 blobs
        b = dc.craft(base, cls=("shift", NATURAL[nc][0]))
        kw.update(fr=list(NATURAL_FRAMES))
    else:
        raise ValueError(case)
    return b, kw


def assert_case(res, A, nc, case):
    assert len(res) == 3
    for s, (tup, n) in enumerate(res):
        if case == "edge":
            assert n == A and tup[0] == min(100, A) and (tup[3] == nc - 1).all()
        elif case == "all":
            assert n == A * nc and tup[0] == min(256, A * nc)
            assert np.array_equal(tup[3], np.tile(np.arange(nc), A)[:tup[0]])       # by anchor, then by class
        elif case == "wide":
            assert n == A * nc and 0 < tup[0] <= 100
            assert np.array_equal(tup[3][:nc], np.arange(nc)) and (tup[4][:nc] == 0).all()      # anchor 0 heads the list: nothing suppresses its nc classes
            assert tup[3].max() < nc and set(tup[3].tolist()) == set(range(nc))
        elif case == "natural":
            lo, hi = natural_band(A, nc)
            w_hi, w_lo = NATURAL[nc][1][{84: 64, 189: 96}[A]][1][s]
            if lo <= w_hi and w_lo <= hi:                      # a frame the CPU table holds inside the band
                assert lo <= n <= hi, (s, n, lo, hi)
            assert tup[3].size == 0 or tup[3].max() < nc


STEP_CASES = [(eid, p, case) for eid in ("64x3", "96x3") for p in PAIRS for case in ("edge", "all", "wide", "natural") if case != "natural" or p[1] == 8]


@pytest.mark.parametrize("eid,pair,case", STEP_CASES, ids=[f"{eid}-{cc.pair_id(p)}-{case}" for eid, p, case in STEP_CASES])
def test_step_on_crafted_finals(capsys, eid, pair, case):
    nc, nk = pair
    W, H = ENGINES[eid][:2]
    b, kw = crafted(nc, nk, case, W, H)
    res, A = run_case(capsys, f"class counts {eid} nc {nc} nk {nk} {case}", b, eid, **kw)
    assert_case(res, A, nc, case)
    if case == "natural":
        assert sum(natural_band(A, nc)[0] <= n <= natural_band(A, nc)[1] for _, n in res) >= 2


@pytest.mark.parametrize("pair", PAIRS, ids=cc.pair_id)
@pytest.mark.parametrize("switch", SWITCHES)
def test_other_producers(capsys, switch, pair):
    """IRMV_EMIT_SCAN=0 (scan_decode_kernel finds a step's candidates), IRMV_SPLIT_SCAN=0 (scan_quad inside nms_pnp_kernel),
    IRMV_SPARSE_HEAD=0 (every row stored)."""
    nc, nk = pair
    W, H = ENGINES["64x3"][:2]
    for case in ("edge", "all"):
        b, kw = crafted(nc, nk, case, W, H)
        res, A = run_case(capsys, f"class counts 64x3 nc {nc} nk {nk} {case} {switch}=0", b, "64x3", switch=switch, **kw)
        assert_case(res, A, nc, case)


def test_results_report_classes_14_and_15_as_unknown(capsys):
    """include/irmv_hip.h, irmv_det.class_id: 0 .. 13, 14 = UNKNOWN.  After `all` at nc = 16 the raw classes of the first 256
    candidates are 0 .. 15 of anchors 0 .. 15; results() reports min(class, 14)."""
    nc, nk = 16, 8
    b, _ = crafted(nc, nk, "all", 64, 64)
    with engine(b, "64x3", max_det=256) as e:
        for s in range(e.num_slots):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(3 + s)
        e.submit(0, e.num_slots)
        e.wait()
        for s in range(e.num_slots):
            raw, arm = e.read_raw(s), e.results(s)
            assert raw["num_dets"] == len(arm) == 256
            assert {14, 15} <= set(raw["classes"].tolist()) and raw["classes"].max() == 15
            assert [int(a.armor_class) for a in arm] == np.minimum(raw["classes"], 14).tolist()


# ---- 3. the layers themselves -------------------------------------------------------------------------------------------------
LAYER_NCS = (1, 5, 16)


@pytest.mark.parametrize("nc", LAYER_NCS)
def test_every_conv_candidate_at_this_class_count(capsys, nc):
    t0 = time.time()
    b = cc.blob(nc)
    finals = [f"model.22.cv3.{i}.2" for i in range(3)]
    table = layer_table(b)
    for name in finals:
        assert table[name][0].shape[0] == nc and table[name][1].shape == (nc,)
    lines = []
    with engine(b, "96x3") as e:
        load_frames(e, e.num_slots)
        res = sweep(e, b, lines.append)
        ops ={op.layer.decode(): op for op in conv_ops(e)}
        carriers = {op.fuse_layer.decode(): name for name, op in ops.items() if op.fused}
    with capsys.disabled():
        print("\n".join(lines))
        print(f"  class finals: " + ", ".join(f"{n} cout {ops[n].cout} pad {ops[n].cout_pad} (fused into {carriers.get(n, '-')})" for n in finals if n in ops))
    _report(f"96x3 nc {nc}", res, t0, capsys)
    worst = res[3]
    for i, name in enumerate(finals):
        assert name in ops and name in worst, name                       # the final was checked against the fp64 reference
        assert ops[name].cout == nc and ops[name].cout_pad == 16 and ops[name].out_f32
        assert f"model.22.cv3.{i}.1" in worst


@pytest.mark.parametrize("nc", LAYER_NCS)
def test_head_against_the_fp32_oracle(capsys, nc):
    b = cc.blob(nc)
    net = oracle.Net(b)
    errs = []
    with engine(b, "96x3") as e:
        for s in range(e.num_slots):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(3 + s)
        e.submit(0, e.num_slots)
        e.wait()
        for s in range(e.num_slots):
            head = e.read_head(s)
            ref = net.forward(oracle.preprocess(frames.synthetic_frame(3 + s), 96))
            assert head.shape == ref.shape == (e.num_anchors, 64 + nc + 8) and e.num_anchors == 189
            errs.append(float(np.abs(head - ref).max()))
            raw, exp = e.read_raw(s), decode(head, 96, 96, nc, 8)
            same_raw(raw, exp, 8, s)
    with capsys.disabled():
        print(f"\n[class counts: head nc {nc}] max|d| vs the fp32 oracle per frame {', '.join(f'{v:.4f}' for v in errs)} (HEAD_TOL {HEAD_TOL})")
    assert max(errs) <= HEAD_TOL


# ---- 4. class policy -----------------------------------------------------------------------------------------------------------
def policy_closed(nc, pol, W, H, kp, md):
    """The closed form of the `all` blob under a policy: the biases with the classes the policy switches off erased."""
    t = cp.min_score_thr(pol, nc)
    if t is None:
        return None
    logit, _ = cp.table(pol, nc)
    bias = cc.all_lit_bias(nc)
    erased = np.where(bias > logit[:nc], bias, dc.DARK).astype(np.float32)
    return dc.closed_form(W, H, erased, 0, kp, t, md, 4096)


@pytest.mark.parametrize("nc", NCS)
def test_class_policy_at_this_class_count(capsys, nc):
    nk, md = 8, 256
    W, H = ENGINES["64x3"][:2]
    kp = dc.quad_kpt_bias(nk)
    b, _ = crafted(nc, nk, "all", W, H)
    off, only = cc.last_off_policy(nc), cc.only_last_policy(nc)
    res, A = run_policy(capsys, f"nc {nc} class {nc - 1} off, 64x3", b, "64x3", off, nc=nc, nk=nk, max_det=md, closed=policy_closed(nc, off, W, H, kp, md))
    for tup, n in res:
        assert n == A * (nc - 1) and tup[0] == min(md, n) and (tup[3] < nc - 1).all()
    res, A = run_policy(capsys, f"nc {nc} only class {nc - 1} on, 64x3", b, "64x3", only, nc=nc, nk=nk, max_det=md, closed=policy_closed(nc, only, W, H, kp, md))
    for tup, n in res:
        assert n == A and tup[0] == min(md, A) and (tup[3] == nc - 1).all()
    if nc == 1:     # the only class off on a batched share: check_policy_step holds every box row of the step to the decoy written before it
        res, A = run_policy(capsys, "nc 1 class 0 off, 96x3", dc.craft(cc.blob(1), cls=("bias", cc.all_lit_bias(1)), box=("bias", dc.POINT_BOXES), kpt=("bias", kp)),
                            "96x3", off, nc=nc, nk=nk, max_det=md)
        assert all(n == 0 and tup[0] == 0 for tup, n in res)
    # run_post on random heads under the first policy
    rng = np.random.default_rng(60 + nc)
    with policy_engine(b, "64x3", max_det=md) as e:
        e.set_class_policy(off)
        A, no = e.num_anchors, e.head_channels
        assert no == 64 + nc + nk
        heads = [(rng.standard_normal((A, no)) * 2).astype(np.float32) for _ in range(e.num_slots)]
        for s, head in enumerate(heads):
            e.write_head(head, s)
        e.run_post(0, e.num_slots)
        total = 0
        for s, head in enumerate(heads):
            exp = reference(e.read_head(s), off, W, H, nc, nk, md, 4096)
            same_raw(e.read_raw(s), exp, nk, s)
            assert exp["n_candidates"] == int(cp.passes(head, off, nc).sum())
            total += exp["n_candidates"]
        assert (total > 0) == (nc > 1)
