"""Class policy on the GPU: per-class score thresholds, the colour mask and the per-class plate, through every candidate
producer.

The reference is always the CPU oracle on the ERASED head: the dense head is read back (read_head), every class logit that
fails its own class's threshold is set to class_policy.DARK (class_policy.erase), and oracle.decode_nms runs at the smallest
enabled threshold.  Erasing states the policy exactly -- the erased pairs are no candidates, the others keep their values --
so read_raw is compared field by field, as tests/test_gpu_detect_craft.py::check_step does, with no condition on the caps.
On engines that store head rows sparsely the raw storage is checked as well: a row whose only passing classes are off must
still hold the decoy written before the step (a masked class set no bit), and the candidate bitmap is all zero afterwards.

The engines are those of tests/test_gpu_detect_craft.py's table, untuned (IRMV_AUTOTUNE=0): 64x3 single-frame steps and the
grouped Detect launch, 96x3 one batched share, 416x4 two stream shares, 640x1 the carriers of 80 x 80 maps.
Pose of the plate test: bit for bit against irmv_pnp_solve on the reported kpts with the class's plate, and 1e-6 on rvec /
tvec against oracle.solve_pnp_ippe.  tests/test_gpu_pnp.py's own bar (pnp_ref.check against an mpmath run per quad) belongs to
a different reference, pnp_ref, and takes seconds per quad; for oracle.solve_pnp_ippe the figure the suite already holds the
fused solver to is 1e-6 (tests/test_gpu_engine.py::test_fused_pnp_matches_oracle, test_gpu_detect_craft.check_results), so
that one is used and no new tolerance is introduced.
Wall time of the module on an MI355X: 29 tests, 10.3 s together, the slowest 1.1 s.
"""
import ctypes as C
import contextlib
import time

import numpy as np
import pytest

import detect_craft as dc
import test_gpu_window as tw
from conftest import D_REF, K_REF
from irmv_detection_amd import arch, capi, class_policy as cp, frames, weights
from irmv_detection_amd.engine import PnPSolver, YoloEngine
from oracle import oracle
from test_class_policy import MASKED_DENSITY, MASKED_NC, density_policy
from test_gpu_detect_craft import ENGINES, SRC, SWITCHES, decode, env, forms_of, storage
from test_gpu_engine import _raw_tuple

pytestmark = pytest.mark.gpu

NC, NK = 14, 8
LADDER_T = (0.1, 0.2, 0.3, 0.4, 0.55, 0.7, 0.85)      # seven different thresholds for classes 0 .. 6


@contextlib.contextmanager
def engine(blob, eid, switch=None, **kw):
    """An engine of test_gpu_detect_craft.ENGINES, always untuned."""
    W, H, S, streams, _ = ENGINES[eid]
    pins = dict(IRMV_AUTOTUNE="0", IRMV_GROUP_FORCE="1")
    pins.update({k: None for k in SWITCHES})
    if switch:
        pins[switch] = "0"
    with env(**pins):
        e = YoloEngine(None, SRC, weights_blob=blob, net_size=W, net_height=None if H == W else H, num_slots=S, num_streams=streams, **kw)
    try:
        yield e
    finally:
        e.close()


def reference(head, pol, W, H, nc, nk, max_det, pre_nms_cap):
    """The CPU oracle on the erased head, at the smallest enabled threshold; every class off: nothing."""
    t = cp.min_score_thr(pol, nc)
    if t is None:
        return dict(n_candidates=0, num_dets=0, anchors=np.zeros(0, np.int32), classes=np.zeros(0, np.int32), boxes=np.zeros((0, 4), np.float32),
                    scores=np.zeros(0, np.float32), kpts=np.zeros((0, nk), np.float32))
    return decode(cp.erase(head, pol, nc), W, H, nc, nk, score_thr=t, max_det=max_det, pre_nms_cap=pre_nms_cap)


def same_raw(raw, exp, nk, where):
    n = raw["num_dets"]
    assert raw["n_candidates"] == exp["n_candidates"], (where, raw["n_candidates"], exp["n_candidates"])
    assert n == exp["num_dets"], (where, n, exp["num_dets"])
    for key in ("anchors", "classes", "boxes", "scores"):
        assert np.array_equal(raw[key], exp[key]), (where, key)
    assert np.array_equal(raw["kpts"][:, :nk], exp["kpts"]), where
    assert not raw["boxes_padded"][n:].any() and not raw["scores_padded"][n:].any(), where


def fill_synthetic(e, s, i):
    e.get_src_image_buffer(s)[:] = frames.synthetic_frame(i)


def check_policy_step(e, pol, fr, log, nc=NC, nk=NK, max_det=100, pre_nms_cap=4096, closed=None, forms=None, fill=fill_synthetic, repeat=True):
    """One step per launch form under the policy in force (pol: its class_policy dict): decoy heads first, then the step, then
    every field of read_raw against the oracle on the erased head; bitmap zero; sparse storage.  -> [(raw tuple, n_candidates)]
    of the first form."""
    W, H = e.net_width, e.net_height
    A, no = e.num_anchors, e.head_channels
    sparse = e.debug_cand_bits(0)[0]
    all_forms, share = forms_of(e)
    names = [k["name"] for k in e.profile(0, min(share, e.num_slots))] if sparse else []
    kpt3 = sum(n.startswith("kpt3") for n in names) == 3
    result = None
    for fi, (first, count) in enumerate(forms or all_forms):
        slots = range(first, first + count)
        decoy = {s: dc.decoy_head(A, no, nc, 1000 * fi + s) for s in slots}
        for s in slots:
            e.write_head(decoy[s], s)
            fill(e, s, fr[s])
        e.submit(first, count)
        e.wait()
        raws = {s: e.read_raw(s) for s in slots}
        for s in range(e.num_slots):
            assert not e.debug_cand_bits(s)[1].any(), (first, count, s)
        stored = storage(e, first, count, nc, nk) if sparse else None
        heads = {s: e.read_head(s).copy() for s in slots}
        out = []
        for k, s in enumerate(slots):
            raw, head = raws[s], heads[s]
            exp = reference(head, pol, W, H, nc, nk, max_det, pre_nms_cap)
            plain_n = int((head[:, 64:64 + nc] > cp.table(cp.uniform(float(pol["score_thr"][:nc].min())), nc)[0][:nc]).sum())
            log(f"    slots {first}..{first + count - 1} slot {s}: n_candidates {raw['n_candidates']} (oracle on the erased head "
                f"{exp['n_candidates']}; {plain_n} pairs above the smallest threshold), num_dets {raw['num_dets']}")
            same_raw(raw, exp, nk, (first, count, s))
            if closed is not None:
                assert raw["n_candidates"] == closed["n_candidates"] and raw["num_dets"] == closed["num_dets"]
                for key in ("anchors", "classes", "boxes", "kpts"):
                    assert np.array_equal(raw[key], closed[key]), (s, key)
            if sparse:
                st, dy = stored[k], decoy[s]
                cand = cp.passes(head, pol, nc).any(1)                 # anchors with a class that passes its OWN threshold
                for name, c in (("box", slice(0, 64)), ("kpt", slice(64 + nc, no))):
                    if c.start == c.stop:
                        continue
                    assert np.array_equal(st[cand][:, c], head[cand][:, c]), (s, name, "a candidate anchor's row is not the dense one")
                    is_decoy = (st[:, c] == dy[:, c]).all(1)
                    is_dense = (st[:, c] == head[:, c]).all(1)
                    assert (is_decoy | is_dense).all(), (s, name)
                    if min(count, share) > 1 and (name == "box" or kpt3):      # the marked carriers of a batched step store candidate rows only
                        assert is_decoy[~cand].all(), (s, name, "a row without a passing class was stored: a masked class set a bit")
            out.append((_raw_tuple(raw), raw["n_candidates"]))
        if repeat:
            e.submit(first, count)
            e.wait()
            for k, s in enumerate(slots):
                again = e.read_raw(s)
                a, b = out[k][0], _raw_tuple(again)
                assert again["n_candidates"] == out[k][1] and a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), (s, "second step differs")
        if fi == 0:
            result = out
    return result


def run(capsys, tag, blob, eid, pol, fr=None, switch=None, engine_kw=None, **kw):
    t0, lines = time.time(), []
    engine_kw = dict(engine_kw or {})
    for k in ("max_det", "pre_nms_cap"):
        if k in kw:
            engine_kw[k] = kw[k]
    try:
        with engine(blob, eid, switch, **engine_kw) as e:
            g0 = e.debug_graph_count()
            e.set_class_policy(pol)
            assert e.debug_graph_count() == g0
            got = e.get_class_policy()
            assert np.array_equal(got["score_thr"], pol["score_thr"]) and np.array_equal(got["plate"], pol["plate"])
            lines.append(f"  engine {eid}: {e.num_slots} slots on {e.num_streams} streams, sparse head {e.debug_cand_bits(0)[0]}")
            lines.append("  class carriers: " + ", ".join(sorted({k["name"] for k in e.profile(0, min(forms_of(e)[1], e.num_slots)) if ".cv3." in k["layer"] or "cv3" in k["name"]})))
            res = check_policy_step(e, pol, fr or [3 + s for s in range(e.num_slots)], lines.append, **kw)
            A = e.num_anchors
    finally:
        with capsys.disabled():
            print(f"\n[class policy: {tag}] {time.time() - t0:.1f} s\n" + "\n".join(lines))
    return res, A


def det_bytes(e, slot=0):
    """Every irmv_det field of the slot's results, as bytes."""
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_results(e._h, slot, e._dets, e.max_det, C.byref(n)))
    return [bytes(e._dets[i]) for i in range(n.value)]


# ---- 1. uniform is a no-op ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid", ["64x3", "416x4"])
def test_uniform_policy_is_a_no_op(blob, eid):
    snaps = []
    with engine(dc.craft(blob, cls=("shift", 3.0)), eid) as e:      # (shifted: every frame has detections to compare)
        S = e.num_slots
        for s in range(S):
            fill_synthetic(e, s, 3 + s)
        for step, setter in enumerate((None, lambda: e.set_class_policy(cp.uniform(0.25, capi.ARMOR_SMALL)), lambda: e.set_class_policy(None, None))):
            g0 = e.debug_graph_count()
            if setter:
                setter()
                assert e.debug_graph_count() == g0
            e.submit(0, S)
            e.wait()
            snaps.append([(_raw_tuple(e.read_raw(s)), e.read_raw(s)["n_candidates"], det_bytes(e, s), e.read_head(s).copy()) for s in range(S)])
            if step:
                assert e.debug_graph_count() == graphs            # the calls and the steps behind them captured nothing new
            graphs = e.debug_graph_count()
        p = e.get_class_policy()
        assert np.all(p["score_thr"] == np.float32(0.25)) and not p["plate"].any()
    assert any(sl[0][0] > 0 for sl in snaps[0])
    for other in snaps[1:]:
        for a, b in zip(snaps[0], other):
            assert a[1] == b[1] and a[0][0] == b[0][0] and all(np.array_equal(x, y) for x, y in zip(a[0][1:], b[0][1:]))
            assert a[2] == b[2] and np.array_equal(a[3], b[3])


# ---- 2. per-class ladder -------------------------------------------------------------------------------------------------------
def ladder_policy_and_bias():
    thr = np.full(16, 0.25, np.float32)
    thr[:7] = LADDER_T
    pol = cp.policy(thr)
    bias = np.full(NC, dc.DARK, np.float32)
    for c, k in enumerate(range(-3, 4)):
        bias[c] = dc.nextafter_k(dc.logit_thr(LADDER_T[c]), k)
    return pol, bias


@pytest.mark.parametrize("eid", ["64x3", "96x3", "416x4", "640x1"])
def test_per_class_ladder(blob, capsys, eid):
    """Class c of 0 .. 6 sits k = c - 3 ulps from ITS OWN threshold: 0 .. 2 below, 3 exactly on it (no candidate), 4 .. 6 one,
    two and three ulps above.  Point boxes: nothing is suppressed, so the survivors are the closed form of the erased biases."""
    W, H = ENGINES[eid][:2]
    pol, bias = ladder_policy_and_bias()
    logit, mn = cp.table(pol, NC)
    assert np.array_equal(bias[:7] > logit[:7], [False] * 4 + [True] * 3) and bias[3] == logit[3] and len(set(LADDER_T)) == 7
    assert (bias[:3] > mn).any()                      # a class below its own threshold is above the smallest one: the pre-test alone would let it through
    kp = dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", bias), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
    erased = np.where(bias > logit[:NC], bias, dc.DARK).astype(np.float32)
    cf = dc.closed_form(W, H, erased, 0, kp, cp.min_score_thr(pol, NC), 256, 4096)
    res, A = run(capsys, f"ladder {eid}", b, eid, pol, max_det=256, closed=cf)
    for tup, n in res:
        assert n == 3 * A and tup[0] == min(256, 3 * A) and set(tup[3].tolist()) <= {4, 5, 6} and tup[3][0] == 6


def test_per_class_ladder_on_the_resident_weight_carriers(blob, capsys):
    """The class carriers a tuned 640 engine runs: the weights-resident kernels (IRMV_FORCE_WRES=3 selects them without the
    tuner, as tests/test_gpu_sparse_branch.py does) -- the ping-pong form on the 80 x 80 map, lockstep on the other levels --
    on three slots over two streams.  25 200 candidates per frame: more than the key list's sort holds."""
    pol, bias = ladder_policy_and_bias()
    kp = dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", bias), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
    logit, _ = cp.table(pol, NC)
    erased = np.where(bias > logit[:NC], bias, dc.DARK).astype(np.float32)
    cf = dc.closed_form(640, 640, erased, 0, kp, cp.min_score_thr(pol, NC), 256, 4096)
    lines = []
    with env(IRMV_AUTOTUNE="0", IRMV_FORCE_WRES="3", **{k: None for k in SWITCHES}):
        e = YoloEngine(None, SRC, weights_blob=b, num_slots=3, num_streams=2, max_det=256)
    try:
        names = {k["layer"]: k["name"] for k in e.profile(0, 2)}
        carriers = {l: n for l, n in names.items() if l.startswith("model.22.cv3.") and l.endswith(".1")}
        lines.append(f"  class carriers: {carriers}")
        e.set_class_policy(pol)
        res = check_policy_step(e, pol, [3, 4, 5], lines.append, max_det=256, closed=cf)
    finally:
        e.close()
        with capsys.disabled():
            print("\n[class policy: ladder, resident weights]\n" + "\n".join(lines))
    assert len(carriers) == 3 and "_wres_pp" in carriers["model.22.cv3.0.1"] and all("_wres" in n and "+1x1" in n for n in carriers.values()), carriers
    for tup, n in res:
        assert n == 3 * 8400 > capi.CAND_CAP and tup[0] == 256 and set(tup[3].tolist()) <= {4, 5, 6} and tup[3][0] == 6


# ---- 3. colour mask -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid", ["64x3", "416x4"])
def test_colour_mask(blob, capsys, eid):
    W, H = ENGINES[eid][:2]
    cls, kp = dc.two_tied_bias(NC, classes=(4, 9)), dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
    for colour, keep in ((0, {4}), (1, {9}), (-1, {4, 9})):
        res, A = run(capsys, f"colour {colour} {eid}", b, eid, cp.enemy(colour, 0.25), max_det=256)
        for tup, n in res:
            assert n == len(keep) * A and tup[0] == min(256, n) and set(tup[3].tolist()) == keep
    res, A = run(capsys, f"all off {eid}", b, eid, cp.uniform(1.0), max_det=256)
    for tup, n in res:
        assert n == 0 and tup[0] == 0


def test_set_enemy_color_is_the_enemy_policy(blob):
    cls = dc.two_tied_bias(NC, classes=(4, 9))
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.POINT_BOXES))
    with engine(b, "64x3", score_thr=0.3) as e:
        fill_synthetic(e, 0, 3)
        for colour, keep in ((0, {4}), (1, {9}), (-1, {4, 9})):
            e.set_enemy_color(colour)
            got, ref = e.get_class_policy(), cp.enemy(colour, 0.3)
            assert np.array_equal(got["score_thr"], ref["score_thr"]) and np.array_equal(got["plate"], ref["plate"])
            assert {int(d.class_id) for d in e.detect(0)} == keep
        with pytest.raises(capi.IrmvError):
            e.set_enemy_color(2)
        assert {int(d.class_id) for d in e.detect(0)} == {4, 9}
        # the colour and the caller's thresholds are independent: class 4 (score 0.78) on a threshold of its own
        thr = np.full(16, 0.3, np.float32)
        thr[4] = 0.9
        e.set_enemy_color(1)
        e.set_class_policy(thr)                               # the colour stays
        assert {int(d.class_id) for d in e.detect(0)} == {9}
        for colour, keep in ((0, set()), (-1, {9}), (1, {9})):
            e.set_enemy_color(colour)                         # ... and so does the threshold
            got = e.get_class_policy()["score_thr"]
            assert got[4] == (np.float32(0.9) if colour != 1 else 1) and (got[9] >= 1) == (colour == 0)
            assert {int(d.class_id) for d in e.detect(0)} == keep
        thr[4] = 0.3
        e.set_class_policy(thr)
        assert {int(d.class_id) for d in e.detect(0)} == {9}
        e.set_class_policy(None, None)                        # back to the constructor's, no colour
        assert {int(d.class_id) for d in e.detect(0)} == {4, 9}


# ---- 4. density under a mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta,fr,want", MASKED_DENSITY, ids=[f"{d:+g}" for d, _, _ in MASKED_DENSITY])
def test_density_under_a_mask(blob, capsys, delta, fr, want):
    """test_class_policy.MASKED_DENSITY: 416x4 with the class finals shifted, under the blue mask and one raised threshold, a
    case per band of detect_craft.bands -- 0 and tens, 513 - 1024 (the lazy-matrix walk of crowded frames), 1025 - 4096,
    4097 - 8192 (the prefilter restart), more than 8192 (the radix select), all pairs of the enabled classes.  Every slot's
    count is the oracle's on the erased head (check_policy_step) and must lie in the band the table gives that slot, which
    tests/test_class_policy.py holds to the CPU oracle with a margin."""
    assert {b for _, _, w in MASKED_DENSITY for b in w} == set(dc.bands(1, MASKED_NC))
    res, A = run(capsys, f"density delta {delta:+g}", dc.craft(blob, cls=("shift", delta)), "416x4", density_policy(), fr=list(fr))
    assert len(res) == len(want) == 4
    for (tup, n), band in zip(res, want):
        lo, hi = dc.bands(A, MASKED_NC)[band]
        assert lo <= n <= hi, (delta, n, band)
        if band == "all":
            assert n == A * MASKED_NC > capi.CAND_CAP
        if band == "0":
            assert n == 0 and tup[0] == 0


# ---- 5. the other producers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", SWITCHES)
def test_other_producers(blob, capsys, switch):
    """IRMV_EMIT_SCAN=0 (scan_decode_kernel), IRMV_SPLIT_SCAN=0 (scan_quad inside nms_pnp_kernel), IRMV_SPARSE_HEAD=0."""
    pol, bias = ladder_policy_and_bias()
    b = dc.craft(blob, cls=("bias", bias))
    res, A = run(capsys, f"ladder 416x4 {switch}=0", b, "416x4", pol, switch=switch)
    for tup, n in res:
        assert n == 3 * A and set(tup[3].tolist()) <= {4, 5, 6}
    res, A = run(capsys, f"density 416x4 {switch}=0", dc.craft(blob, cls=("shift", 4.5)), "416x4", density_policy(), fr=[1, 3, 6, 11], switch=switch)
    assert all(n > 512 for _, n in res)


@pytest.mark.parametrize("switch", [None, "IRMV_SPLIT_SCAN"])
def test_run_post_on_a_random_head_obeys_the_policy(blob, switch):
    rng = np.random.default_rng(11)
    pol = density_policy()
    pol["score_thr"][5] = np.float32(0.9)
    with engine(blob, "96x3", switch) as e:
        e.set_class_policy(pol)
        W, H, A, no = e.net_width, e.net_height, e.num_anchors, e.head_channels
        for s in range(e.num_slots):
            head = (rng.standard_normal((A, no)) * 2).astype(np.float32)
            head[:, 64:64 + NC] -= np.float32(1.5 * s)
            e.write_head(head, s)
        e.run_post(0, e.num_slots)
        for s in range(e.num_slots):
            head = e.read_head(s)
            exp = reference(head, pol, W, H, NC, NK, 100, 4096)
            assert exp["n_candidates"] > 0 or s > 0
            same_raw(e.read_raw(s), exp, NK, s)


def test_shufflenet_int8_blob(capsys):
    pol, bias = ladder_policy_and_bias()
    b = dc.craft(weights.quantize_blob_int8(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)), cls=("bias", bias))
    res, A = run(capsys, "ladder 416x4 shufflenet int8", b, "416x4", pol)
    for tup, n in res:
        assert n == 3 * A


def test_bbox_only_blob(capsys):
    pol, bias = ladder_policy_and_bias()
    b = dc.craft(weights.synthetic_blob(0, nk=0), cls=("bias", bias))
    res, A = run(capsys, "ladder 96x3 nk 0", b, "96x3", pol, nk=0)
    for tup, n in res:
        assert n == 3 * A


# ---- 6. live change -------------------------------------------------------------------------------------------------------------
def test_live_change_between_steps_in_flight(blob):
    cls = dc.two_tied_bias(NC, classes=(4, 9))
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.POINT_BOXES), kpt=("bias", dc.quad_kpt_bias(8)))
    with engine(b, "416x4", max_det=256) as e:
        S, share = e.num_slots, 2
        for s in range(S):
            fill_synthetic(e, s, 3 + s)

        def classes_after(submits):
            for first, count in submits:
                e.submit(first, count, async_upload=True)      # in flight: nothing waits here

        classes_after([(0, share), (share, share)])
        e.set_class_policy(cp.enemy(0, 0.25))                  # waits for both, then writes the table
        first = [set(e.read_raw(s)["classes"].tolist()) for s in range(S)]
        graphs = e.debug_graph_count()
        classes_after([(0, share), (share, share)])
        e.set_class_policy(cp.enemy(1, 0.25))
        second = [set(e.read_raw(s)["classes"].tolist()) for s in range(S)]
        classes_after([(0, share), (share, share)])
        e.wait()
        third = [set(e.read_raw(s)["classes"].tolist()) for s in range(S)]
        assert e.debug_graph_count() == graphs
        assert first == [{4, 9}] * S and second == [{4}] * S and third == [{9}] * S
        n = [e.read_raw(s)["n_candidates"] for s in range(S)]
        assert n == [e.num_anchors] * S


def test_window_engine_keeps_the_policy_across_set_window_and_set_view(blob, capsys):
    cls = dc.two_tied_bias(NC, classes=(4, 9))
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.POINT_BOXES), kpt=("bias", dc.quad_kpt_bias(8)))
    full, win, net = (256, 128), (128, 64), (128, 64)
    pol = cp.enemy(1, 0.25)
    lines = []
    fill = lambda e, s, i: e.get_src_image_buffer(s).__setitem__(slice(None), tw.frame_of(i, full))
    with env(IRMV_AUTOTUNE="0"):
        e = YoloEngine(None, full, weights_blob=b, net_size=net[0], net_height=net[1], window=win, num_slots=2, max_det=256)
    try:
        e.set_view("frame", 0); e.set_view("window", 0)        # build the frame view before counting graphs
        e.set_class_policy(pol)
        for step, act in enumerate((lambda: None, lambda: [e.set_window(5, 7, s) for s in range(2)], lambda: [e.set_view("frame", s) for s in range(2)],
                                    lambda: [e.set_view("window", s) for s in range(2)])):
            act()
            res = check_policy_step(e, pol, [0, 1], lines.append, max_det=256, forms=[(0, 2)], fill=fill, repeat=False)
            for tup, n in res:
                assert n == e.num_anchors and set(tup[3].tolist()) == {9}
            if step == 3:
                assert e.debug_graph_count() == graphs
            if step == 2:
                graphs = e.debug_graph_count()
        g = e.debug_graph_count()
        e.set_class_policy(cp.enemy(0, 0.25))
        assert e.debug_graph_count() == g
        res = check_policy_step(e, cp.enemy(0, 0.25), [0, 1], lines.append, max_det=256, forms=[(0, 2)], fill=fill, repeat=False)
        assert all(set(tup[3].tolist()) == {4} for tup, _ in res) and e.debug_graph_count() == g
    finally:
        e.close()
        with capsys.disabled():
            print("\n[class policy: window engine]\n" + "\n".join(lines))


def test_profile_under_a_policy_leaves_nothing_behind(blob, capsys):
    """irmv_engine_profile repeats every launch; the muted repetitions of the class carriers must stay mute under a policy."""
    pol, bias = ladder_policy_and_bias()
    b = dc.craft(blob, cls=("bias", bias))
    lines = []
    with engine(b, "416x4") as e:
        assert e.debug_cand_bits(0)[0]
        e.set_class_policy(pol)
        for s in range(e.num_slots):
            fill_synthetic(e, s, 3 + s)
        for first, count in ((0, 2), (0, 4), (3, 1)):
            stats = e.profile(first, count)
            assert any(k["name"].startswith("nms") for k in stats)
            for s in range(e.num_slots):
                assert not e.debug_cand_bits(s)[1].any(), (first, count, s)
            for s in range(first, first + count):
                assert e.read_raw(s)["n_candidates"] == 3 * e.num_anchors      # counted once: the muted repetitions appended nothing
        res = check_policy_step(e, pol, [3, 4, 5, 6], lines.append)
        assert all(n == 3 * e.num_anchors for _, n in res)
    with capsys.disabled():
        print("\n[class policy: profile]\n" + "\n".join(lines))


# ---- 7. plate per class, keypoint path -------------------------------------------------------------------------------------------
def test_plate_per_class_keypoint_path(blob):
    cls, kp = dc.two_tied_bias(NC, classes=(4, 9)), dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
    plate = np.zeros(16, np.uint8)
    plate[4] = capi.ARMOR_LARGE
    solver = PnPSolver(K_REF, list(D_REF))
    with engine(b, "96x3", max_det=256) as e:
        fill_synthetic(e, 0, 3)
        e.detect(0)
        before = e.results(0)
        assert {int(a.size) for a in before} == {0}
        e.set_class_policy(None, plate)
        assert np.all(e.get_class_policy()["score_thr"] == np.float32(0.25))
        e.detect(0)
        arm = e.results(0)
        raw = e.read_raw(0)
    assert len(arm) == len(before) == 256 and {int(a.armor_class) for a in arm} == {4, 9}
    assert raw["classes"].tolist() == [int(a.armor_class) for a in arm]
    sizes, n_ok = set(), 0
    for a, a0 in zip(arm, before):
        want = int(plate[int(a.armor_class)])
        assert int(a.size) == want and np.array_equal(a.image_points(), a0.image_points())
        sizes.add(want)
        pts = a.image_points().reshape(1, 8)
        ok, r, t = solver.solve_batch(pts, want)
        assert bool(ok[0]) == a.pnp_ok
        o = oracle.solve_pnp_ippe(K_REF, D_REF, pts[0], want)
        assert o["ok"] == a.pnp_ok
        if a.pnp_ok:
            n_ok += 1
            assert np.array_equal(r[0], a.rvec) and np.array_equal(t[0], a.tvec), (int(a.armor_class), r[0] - a.rvec, t[0] - a.tvec)
            assert np.abs(o["rvec"] - a.rvec).max() <= 1e-6 and np.abs(o["tvec"] - a.tvec).max() <= 1e-6
            q = oracle.rvec_to_quat(a.rvec)
            assert min(np.abs(q - a.quat_xyzw).max(), np.abs(q + a.quat_xyzw).max()) <= 1e-6
            if want == capi.ARMOR_SMALL:      # the small plate's pose is what the uniform engine gave
                assert np.array_equal(a.rvec, a0.rvec) and np.array_equal(a.tvec, a0.tvec) and np.array_equal(a.quat_xyzw, a0.quat_xyzw)
            else:
                assert not np.array_equal(a.tvec, a0.tvec)
    solver.close()
    assert sizes == {0, 1} and n_ok > 0


# ---- 8. plate per class, classical path ------------------------------------------------------------------------------------------
def test_plate_per_class_classical_path(blob, rm_test_image):
    """A policy with every plate LARGE on an engine created SMALL gives every irmv_det field of an engine created LARGE;
    irmv_engine_extract_armors on explicit boxes has no class and keeps cfg.armor_size."""
    import json
    from conftest import golden_path
    boxes = np.array([c["box"] for c in json.load(open(golden_path("light_cases.json")))], np.float32)
    b = dc.craft(blob, cls=("shift", 3.0))
    kw = dict(weights_blob=b, rotate180=False, point_source=capi.POINTS_CLASSICAL, max_det=256)
    out = {}
    for name, size in (("large", capi.ARMOR_LARGE), ("small", capi.ARMOR_SMALL)):
        with env(IRMV_AUTOTUNE="0"):
            e = YoloEngine(None, (1280, 1024), armor_size=size, **kw)
        try:
            e.get_src_image_buffer()[:] = rm_test_image
            e.detect(0)
            out[name] = det_bytes(e)
            out[name + " boxes"] = [bytes(d) for d in e.extract_armors_raw(boxes)][:len(boxes)]
            if name == "small":
                e.set_class_policy(None, capi.ARMOR_LARGE)
                e.detect(0)
                out["policy"] = det_bytes(e)
                out["policy armors"] = e.results(0)
                out["policy boxes"] = [bytes(d) for d in e.extract_armors_raw(boxes)][:len(boxes)]
        finally:
            e.close()
    solved = [a for a in out["policy armors"] if a.pnp_ok]
    print(f"classical path: {len(out['policy'])} detections, {len(solved)} with a solved pose")
    assert len(out["large"]) > 0 and solved                          # the comparison sees poses
    assert out["policy"] == out["large"] and out["policy"] != out["small"]
    assert out["policy boxes"] == out["small boxes"] and out["small boxes"] != out["large boxes"]


# ---- 9. errors on a living engine -------------------------------------------------------------------------------------------------
def test_errors_leave_the_engine_as_it_was(blob):
    b = dc.craft(blob, cls=("shift", 3.0))
    with engine(b, "64x3") as e:
        fill_synthetic(e, 0, 3)
        e.set_enemy_color(0)
        before, pol = (_raw_tuple(e.read_raw(0)) if e.detect(0) is not None else None), e.get_class_policy()
        dets = det_bytes(e)
        assert before[0] > 0
        for bad in (dict(score_thr=[0.25, np.nan]), dict(score_thr=[0.0]), dict(score_thr=-1.0), dict(plate=[0, 2]), dict(plate=7)):
            with pytest.raises(capi.IrmvError) as ei:
                e.set_class_policy(**bad)
            assert ei.value.code == capi.ERR_ARG
            got = e.get_class_policy()
            assert np.array_equal(got["score_thr"], pol["score_thr"]) and np.array_equal(got["plate"], pol["plate"])
        p = capi.class_policy_uniform(0.25)
        p.struct_size = 8
        assert e._L.irmv_engine_set_class_policy(e._h, C.byref(p)) == capi.ERR_ARG
        e.detect(0)
        after = _raw_tuple(e.read_raw(0))
        assert after[0] == before[0] and all(np.array_equal(x, y) for x, y in zip(after[1:], before[1:])) and det_bytes(e) == dets
