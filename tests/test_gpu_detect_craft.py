"""Whole steps on crafted Detect finals (tests/detect_craft.py; proven on the CPU in tests/test_detect_craft.py).

Every other exact test of the post stage writes a head from the host (write_head + run_post): its candidates come from
scan_decode_kernel.  A real step takes them from the class carriers' conv epilogue (threshold compare, atomicAdd on the
frame's counter, key store, atomicOr into the candidate bitmap), stores box and keypoint rows only where the bitmap says
so, and runs its launches in the order sparse_head_plan chose.  A crafted blob -- the class final's weights zeroed, so every
class logit of a level IS that level's bias -- puts a head chosen by the test behind those producers.

check_step() is the one check, run on every case and every launch form (the batched step, then one stream's share alone):
a decoy head is written into every slot first; after the step read_raw must equal the oracle's decode / NMS of the head
read back (n_candidates, num_dets, anchors, classes, boxes, scores, kpts, zero padding) and the closed form where one
exists; the candidate bitmap is all zero; a second identical step gives the same raw tuple; and on engines that store
head rows sparsely the raw storage of head.0 .. head.2 (read before any read-back) holds the dense values in the box and
keypoint columns of every candidate anchor, and still the decoy on every other row of a batched step.

Density cases: class finals shifted by delta, everything else natural.  (delta, frames) and the oracle's counts, from
tests/test_detect_craft.py::test_density_table_sits_inside_its_bands (threshold moved by -/+ HEAD_TOL in brackets):

    416 x 416 x 4   +0.25  frames 3, 0, 2, 4      0, 39, 28, 28                   [0, 39, 26..28, 25..32]
                    +1.75  frames 1, 6, 11, 20    784, 41, 0, 26                  [763..798, 38..46, 0, 25..28]
                    +4.5   frames 1, 3, 6, 11     5057, 2866, 2980, 2623          [4902..5225, 2642..3148, 2849..3298, 2574..2886]
                    +7.75  frames 0, 1, 2, 3      25257, 26915, 23614, 22485      [18942 .. 28609]
                    +30    frames 0, 1, 2, 3      49686 = A nc, each
    640 x 512 x 2   -5     frames 1, 2            39, 0                           [38..39, 0]
                    +0.5   frames 1, 3            758, 30                         [742..772, 28..30]
                    +2.25  frames 1, 5            1963, 797                       [1920..2005, 764..828]
                    +4     frames 0, 2            6207, 5445                      [6093..6320, 5376..5508]
                    +7.75  frames 0, 3            48462, 43636                    [37231 .. 53190]
                    +30    frames 0, 1            94080 = A nc, each

The GPU's own counts are in DESIGN.md (section 14).  Wall time of the module on an MI355X: 45 tests, 14.8 s together, the
slowest 1.2 s.
"""
import contextlib
import os
import time

import numpy as np
import pytest

import detect_craft as dc
import rect_ref
from conftest import D_REF, K_REF
from irmv_detection_amd import arch, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_detect_craft import DENSITY, PAIRS
from test_gpu_engine import _raw_tuple

pytestmark = pytest.mark.gpu

SRC = (1280, 1024)
# id -> (W, H, slots, streams (0: the engine's default), default tuning)
ENGINES = {
    "640x1": (640, 640, 1, 0, True),          # the production tiles: autotuned, grouped only where it timed faster
    "416x4": (416, 416, 4, 2, False),         # two stream shares of two frames: the batched plan
    "96x3": (96, 96, 3, 1, False),            # one share of three
    "64x3": (64, 64, 3, 0, False),            # as many streams as slots: single-frame steps, grouped Detect launches
    "640x512x2": (640, 512, 2, 0, False),
}
SWITCHES = ("IRMV_SPARSE_HEAD", "IRMV_EMIT_SCAN", "IRMV_SPLIT_SCAN")


@contextlib.contextmanager
def env(**kw):
    """Set (value) or unset (None) environment variables the engine reads at creation; restored on exit."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def engine(blob, eid, switch=None, **kw):
    W, H, S, streams, tuned = ENGINES[eid]
    pins = dict(IRMV_AUTOTUNE=None, IRMV_GROUP_FORCE=None) if tuned else dict(IRMV_AUTOTUNE="0", IRMV_GROUP_FORCE="1")
    pins.update({k: None for k in SWITCHES})
    if switch:
        pins[switch] = "0"
    with env(**pins):
        e = YoloEngine(None, SRC, weights_blob=blob, net_size=W, net_height=None if H == W else H, num_slots=S, num_streams=streams, **kw)
    try:
        yield e
    finally:
        e.close()


def decode(head, W, H, nc, nk, **kw):
    return oracle.decode_nms(head, W, nc, nk, **kw) if W == H else rect_ref.decode_nms(head, W, H, nc, nk, **kw)


def forms_of(e):
    """(first, count) of every launch form: the batched step; then one stream's share alone -- the second stream's, or
    where one stream holds every slot, slots 1 .. of it; the last slot of an engine of single-frame shares."""
    S = e.num_slots
    share = -(-S // e.num_streams)
    out = [(0, S)]
    if S > 1:
        out.append((share, min(share, S - share)) if share < S else (1, S - 1))
    return out, share


REC_CLS, REC_KPT = 64, 80      # a stored head record: 96 floats, box 64 | classes at 64 (16 columns) | keypoints at 80 (irmv_common.hpp)


def storage(e, first, count, nc, nk):
    """Raw storage of the head rows of slots [first, first + count), in read_head's column order: [count, A, 64 + nc + nk];
    no read-back step in front (read_head, read_tap and read_tensor all bring a sparse head to the dense state first)."""
    rec = np.stack([e.debug_head_rows(s) for s in range(first, first + count)])
    return np.concatenate([rec[..., :64], rec[..., REC_CLS:REC_CLS + nc], rec[..., REC_KPT:REC_KPT + nk]], -1)


def check_step(e, fr, log, nc=14, nk=8, score_thr=0.25, max_det=100, pre_nms_cap=4096, closed=None, lit=None):
    """The check (module docstring).  fr: frame index per slot.  closed: dict of the closed form's survivors (the same on
    every slot), or None.  lit: the one level that may hold candidates, or None.  -> raw tuple and n_candidates per slot, of
    the batched step."""
    W, H = e.net_width, e.net_height
    A, no = e.num_anchors, e.head_channels
    assert A == sum(dc.level_sizes(W, H)) and no == 64 + nc + nk
    thr = dc.logit_thr(score_thr)
    kw = dict(score_thr=score_thr, max_det=max_det, pre_nms_cap=pre_nms_cap)
    sparse = e.debug_cand_bits(0)[0]
    forms, share = forms_of(e)
    names = [k["name"] for k in e.profile(0, min(share, e.num_slots))] if sparse else []
    kpt3 = sum(n.startswith("kpt3") for n in names) == 3
    bases, sizes = dc.level_bases(W, H), dc.level_sizes(W, H)
    result = None
    for fi, (first, count) in enumerate(forms):
        slots = range(first, first + count)
        decoy = {s: dc.decoy_head(A, no, nc, 1000 * fi + s) for s in slots}
        for s in slots:
            e.write_head(decoy[s], s)
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(fr[s])
        if sparse:
            assert np.array_equal(storage(e, first, count, nc, nk), np.stack([decoy[s] for s in slots]))     # the decoy is what a step finds
        e.submit(first, count)
        e.wait()
        raws = {s: e.read_raw(s) for s in slots}
        arm = {s: e.results(s) for s in slots}
        for s in range(e.num_slots):
            words = e.debug_cand_bits(s)[1]
            assert not words.any(), (first, count, s, np.nonzero(words)[0][:8])
        stored = storage(e, first, count, nc, nk) if sparse else None
        heads = {s: e.read_head(s).copy() for s in slots}
        if sparse:                                      # ... and after the read-back the storage is the dense head
            assert np.array_equal(storage(e, first, count, nc, nk), np.stack([heads[s] for s in slots]))
        out = []
        for k, s in enumerate(slots):
            raw, head = raws[s], heads[s]
            exp = decode(head, W, H, nc, nk, **kw)
            n = raw["num_dets"]
            log(f"    slots {first}..{first + count - 1} slot {s} frame {fr[s]}: n_candidates {raw['n_candidates']} (oracle on the head read back {exp['n_candidates']}), num_dets {n}")
            assert raw["n_candidates"] == exp["n_candidates"], (s, raw["n_candidates"], exp["n_candidates"])
            assert n == exp["num_dets"], (s, n, exp["num_dets"])
            for key in ("anchors", "classes", "boxes", "scores"):
                assert np.array_equal(raw[key], exp[key]), (s, key)
            assert np.array_equal(raw["kpts"][:, :nk], exp["kpts"]), s
            assert not raw["boxes_padded"][n:].any() and not raw["scores_padded"][n:].any()
            if closed is not None:
                assert raw["n_candidates"] == closed["n_candidates"]
                if "num_dets" in closed:
                    assert n == closed["num_dets"]
                    for key in ("anchors", "classes", "boxes"):
                        assert np.array_equal(raw[key], closed[key]), (s, key)
                    assert np.array_equal(raw["kpts"][:, :nk], closed["kpts"]), (s, "kpts")
                else:        # wide boxes: the survivors are the oracle's; their boxes and keypoints are the closed form's
                    assert np.array_equal(raw["boxes"], closed["all_boxes"][raw["anchors"]])
                    assert np.array_equal(raw["kpts"][:, :nk], closed["all_kpts"][raw["anchors"]])
                if nk:       # (a model without a keypoint head takes its points from the light bars, not from the closed form)
                    check_results(arm[s], raw, closed, W, H)
            if lit is not None:
                assert ((raw["anchors"] >= bases[lit]) & (raw["anchors"] < bases[lit] + sizes[lit])).all(), s
            if sparse:
                st, dy = stored[k], decoy[s]
                cand = (head[:, 64:64 + nc] > thr).any(1)
                cols = {"box": slice(0, 64), "cls": slice(64, 64 + nc), "kpt": slice(64 + nc, no)}
                kept = {}
                for name, c in cols.items():
                    if c.start == c.stop:
                        continue
                    if name != "cls":       # (the class columns stay on chip: a sparse step stores none of them)
                        assert np.array_equal(st[cand][:, c], head[cand][:, c]), (s, name, "a candidate anchor's row is not the dense one")
                    is_decoy = (st[:, c] == dy[:, c]).all(1)
                    is_dense = (st[:, c] == head[:, c]).all(1)
                    assert (is_decoy | is_dense).all(), (s, name, "a row that is neither the decoy nor the dense head")
                    kept[name] = int(is_decoy[~cand].sum())
                    if min(count, share) > 1 and (name == "box" or (name == "kpt" and kpt3)):      # the marked carriers of a batched step: nothing but candidate rows is stored
                        assert kept[name] == int((~cand).sum()), (s, name, kept[name], int((~cand).sum()))
                log(f"      sparse: {int(cand.sum())} candidate anchors of {A}; non-candidate rows still the decoy: "
                    + ", ".join(f"{k_} {v}" for k_, v in kept.items()) + f" of {int((~cand).sum())}" + ("" if min(count, share) > 1 else " (single-frame step: logged only)"))
            out.append((_raw_tuple(raw), raw["n_candidates"]))
        e.submit(first, count)              # emission order is atomic order: the result must not depend on it
        e.wait()
        for k, s in enumerate(slots):
            again = e.read_raw(s)
            a, b = out[k][0], _raw_tuple(again)
            assert again["n_candidates"] == out[k][1] and a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), (s, "second step differs")
        for s in range(e.num_slots):
            assert not e.debug_cand_bits(s)[1].any(), s
        if fi == 0:
            result = out
    return result


def check_results(armors, raw, closed, W, H):
    """results(): keypoints in source pixels are the closed form's mapped by the engine's scale; the pose is the oracle's
    on those points (1e-6: test_fused_pnp_matches_oracle)."""
    assert len(armors) == raw["num_dets"]
    want = dc.to_source(closed["all_kpts"][raw["anchors"]], SRC, W, H)
    n_ok = 0
    for a, pts in zip(armors, want):
        assert np.array_equal(a.image_points().reshape(8), pts)
        o = oracle.solve_pnp_ippe(K_REF, D_REF, pts, 0)
        assert o["ok"] == a.pnp_ok
        if a.pnp_ok:
            n_ok += 1
            assert np.abs(o["rvec"] - a.rvec).max() <= 1e-6 and np.abs(o["tvec"] - a.tvec).max() <= 1e-6
    assert n_ok > 0 or not armors


def frames_for(S, base=3):
    return [base + s for s in range(S)]


def run_case(capsys, tag, blob, eid, fr=None, switch=None, engine_kw=None, **kw):
    t0 = time.time()
    lines = []
    engine_kw = dict(engine_kw or {})
    for k in ("score_thr", "max_det", "pre_nms_cap"):
        if k in kw:
            engine_kw[k] = kw[k]
    try:
        with engine(blob, eid, switch, **engine_kw) as e:
            lines.append(f"  engine {eid}: {e.num_slots} slots on {e.num_streams} streams, sparse head {e.debug_cand_bits(0)[0]}")
            res = check_step(e, fr or frames_for(e.num_slots), lines.append, **kw)
            A = e.num_anchors
    finally:
        with capsys.disabled():
            print(f"\n[detect craft: {tag}] {time.time() - t0:.1f} s\n" + "\n".join(lines))
    return res, A


# ---- ladder ------------------------------------------------------------------------------------------------------------
def assert_ladder(res, A):
    for tup, n in res:
        assert n == 3 * A                                   # classes 4, 5, 6 of every anchor; class 3 sits ON the threshold
        assert tup[0] > 0 and set(tup[3].tolist()) <= {4, 5, 6} and tup[3][0] == 6


@pytest.mark.parametrize("eid", list(ENGINES))
def test_ladder(blob, capsys, eid):
    b = dc.craft(blob, cls=("bias", dc.ladder_bias(14)))
    res, A = run_case(capsys, f"ladder {eid}", b, eid)
    assert_ladder(res, A)
    if eid == "640x1":
        assert res[0][1] == 25200 > capi.CAND_CAP           # more tied keys than the key list's sort holds: radix select over atomic order


def test_ladder_without_keypoints(capsys):
    b = dc.craft(weights.synthetic_blob(0, nk=0), cls=("bias", dc.ladder_bias(14)))
    res, A = run_case(capsys, "ladder 96x3 nk 0", b, "96x3", nk=0)
    assert_ladder(res, A)


def test_ladder_on_the_shufflenet_int8_blob(capsys):
    b = dc.craft(weights.quantize_blob_int8(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)), cls=("bias", dc.ladder_bias(14)))
    assert weights.parse_blob(b)[0]["dtype"] == weights.DTYPE_INT8
    res, A = run_case(capsys, "ladder 416x4 shufflenet int8", b, "416x4")
    assert_ladder(res, A)


# ---- zero edge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid", ["416x4", "64x3"])
def test_zero_edge(blob, capsys, eid):
    """score_thr 0.5: logit_thr is exactly 0.  The read-back class columns are the bias as values -- a kernel that flushed the
    subnormal would show a zero here -- and the candidates are the classes whose value is > 0: FLT_MIN, then the subnormal."""
    z, kp = dc.zero_edge_bias(14), dc.quad_kpt_bias(8)
    W, H = ENGINES[eid][:2]
    b = dc.craft(blob, cls=("bias", z), box=("bias", dc.POINT_BOXES), kpt=("bias", kp))
    with engine(b, eid, score_thr=0.5, max_det=256) as e:
        e.get_src_image_buffer(0)[:] = frames.synthetic_frame(3)
        e.detect(0)
        cl = e.read_head(0)[:, 64:78]
    assert np.array_equal(cl, np.broadcast_to(z, cl.shape)), np.nonzero((cl != z).any(0))[0]
    assert (cl[:, 3] > 0).all() and (cl[:, 5] > 0).all()
    cf = dc.closed_form(W, H, z, 0, kp, 0.5, 256, 4096)
    res, A = run_case(capsys, f"zero edge {eid}", b, eid, score_thr=0.5, max_det=256, closed=cf)
    for tup, n in res:
        assert n == 2 * A and set(tup[3].tolist()) <= {3, 5} and tup[3][0] == 5
        if 2 * A <= 256:
            assert sorted(set(tup[3].tolist())) == [3, 5]


# ---- density ------------------------------------------------------------------------------------------------------------
DENSITY_CASES = [(eid, i) for eid, net in (("416x4", (416, 416)), ("640x512x2", (640, 512))) for i in range(len(DENSITY[net]))]


@pytest.mark.parametrize("eid,i", DENSITY_CASES, ids=[f"{eid}-{i}" for eid, i in DENSITY_CASES])
def test_density(blob, capsys, eid, i):
    W, H = ENGINES[eid][:2]
    delta, fr, want = DENSITY[(W, H)][i]
    assert {b for _, _, w in DENSITY[(W, H)] for b in w} == set(dc.bands(1, 14))      # the cases of this net cover every band ...
    res, A = run_case(capsys, f"density {eid} delta {delta:+g}", dc.craft(blob, cls=("shift", delta)), eid, fr=list(fr))
    for (tup, n), band in zip(res, want):
        lo, hi = dc.bands(A, 14)[band]
        assert lo <= n <= hi, (delta, n, band)                                     # ... and each asserts its own on the GPU's count
        if band == "all":
            assert n == A * 14
        if band == "0":
            assert n == 0 and tup[0] == 0


# ---- closed form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid", ["416x4", "64x3"])
@pytest.mark.parametrize("md,cap", PAIRS)
@pytest.mark.parametrize("box_bin", [0, 15])
def test_closed_form(blob, capsys, eid, md, cap, box_bin):
    W, H = ENGINES[eid][:2]
    cls, kp = dc.two_tied_bias(14), dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", cls), box=("bias", dc.dfl_bias(box_bin)), kpt=("bias", kp))
    cf = dc.closed_form(W, H, cls, box_bin, kp, 0.25, md, cap)
    res, A = run_case(capsys, f"closed form {eid} bin {box_bin} max_det {md} cap {cap}", b, eid, max_det=md, pre_nms_cap=cap, closed=cf)
    for tup, n in res:
        assert n == 2 * A
        if box_bin == 0:
            assert tup[0] == min(md, cap, 2 * A)
        else:
            assert 0 < tup[0] <= min(md, cap)


# ---- one level lit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid", ["416x4", "96x3"])
@pytest.mark.parametrize("L", [0, 1, 2])
def test_one_level_lit(blob, capsys, eid, L):
    """Level bases 2704 / 3380 (416) and 144 / 180 (96) are no multiples of 32: two levels share a bitmap word."""
    W, H = ENGINES[eid][:2]
    b = dc.craft(blob, cls={l: ("bias", dc.ladder_bias(14) if l == L else dc.dark_bias(14)) for l in range(3)})
    res, A = run_case(capsys, f"level {L} lit {eid}", b, eid, lit=L)
    for tup, n in res:
        assert n == 3 * dc.level_sizes(W, H)[L] and tup[0] > 0


# ---- other producers ----------------------------------------------------------------------------------------------------
def _producer_blobs(blob):
    cls, kp = dc.two_tied_bias(14), dc.quad_kpt_bias(8)
    return {"ladder": (dc.craft(blob, cls=("bias", dc.ladder_bias(14))), None),
            "closed form, wide": (dc.craft(blob, cls=("bias", cls), box=("bias", dc.WIDE_BOXES), kpt=("bias", kp)),
                                  dc.closed_form(416, 416, cls, 15, kp))}


_default_416 = {}


@pytest.mark.parametrize("switch", SWITCHES)
def test_other_producers(blob, capsys, switch):
    """IRMV_SPARSE_HEAD=0 (every row stored), IRMV_EMIT_SCAN=0 (scan_decode_kernel finds the candidates), IRMV_SPLIT_SCAN=0
    (the scan inside nms_pnp_kernel): the same check, and raw tuples identical to the default engine's."""
    for name, (b, cf) in _producer_blobs(blob).items():
        if name not in _default_416:
            _default_416[name] = run_case(capsys, f"{name} 416x4 default", b, "416x4", closed=cf)[0]
        res, _ = run_case(capsys, f"{name} 416x4 {switch}=0", b, "416x4", switch=switch, closed=cf)
        for s, ((a, na), (d, nd)) in enumerate(zip(res, _default_416[name])):
            assert na == nd and a[0] == d[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], d[1:])), (name, switch, s)
