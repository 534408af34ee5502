"""tests/detect_craft.py against the CPU oracle, before the GPU sees a crafted blob (tests/test_gpu_detect_craft.py).

  * a zero-weight final gives a head equal to its bias, as values, on every anchor: nets 64, 96 and 416 through the fp32
    oracle (oracle/orc_net.c), 640 x 512 through tests/torch_ref.TorchNet (the oracle is square-only);
  * closed_form() equals oracle.decode_nms (rect_ref.decode_nms on the rectangle) on that head, at the four
    (max_det, pre_nms_cap) pairs of the GPU test, for point-like and for wide boxes;
  * the ladder gives exactly 3 A candidates, the zero-edge vector exactly the classes with a bias > 0;
  * DENSITY, the (delta, frames) table of the GPU test's density cases, is computed here: the oracle's candidate count of
    every (delta, frame) pair sits inside its band with 20 % of the band's width clear of either edge, and stays inside it
    when the threshold moves by HEAD_TOL either way -- the GPU's head differs from the oracle's by up to HEAD_TOL, so the
    GPU's own count is bracketed by those two.
"""
import numpy as np
import pytest

import detect_craft as dc
import rect_ref
from irmv_detection_amd import frames, weights
from oracle import oracle
from torch_ref import TorchNet

HEAD_TOL = 4e-2     # tests/test_gpu_engine.py: any frame's max |d head| of the engine against the fp32 oracle
SRC = (1280, 1024)
PAIRS = [(100, 4096), (7, 4096), (256, 150), (256, 4096)]      # (max_det, pre_nms_cap)

# net (W, H) -> [(delta, (frame per slot), (band per slot))]: one engine per delta, a distinct frame in every slot, the slots
# of one batched step in different bands.  The counts are in the module docstring of tests/test_gpu_detect_craft.py.
DENSITY = {
    (416, 416): [(0.25, (3, 0, 2, 4), ("0", "1-64", "1-64", "1-64")),
                 (1.75, (1, 6, 11, 20), ("513-1024", "1-64", "0", "1-64")),
                 (4.5, (1, 3, 6, 11), ("4097-8192", "1025-4096", "1025-4096", "1025-4096")),
                 (7.75, (0, 1, 2, 3), (">8192",) * 4),
                 (30.0, (0, 1, 2, 3), ("all",) * 4)],
    (640, 512): [(-5.0, (1, 2), ("1-64", "0")),
                 (0.5, (1, 3), ("513-1024", "1-64")),
                 (2.25, (1, 5), ("1025-4096", "513-1024")),
                 (4.0, (0, 2), ("4097-8192",) * 2),
                 (7.75, (0, 3), (">8192",) * 2),
                 (30.0, (0, 1), ("all",) * 2)],
}


def oracle_head(blob, W, H, frame):
    """The fp32 reference head of a frame: the C oracle on square nets, TorchNet on the rectangle."""
    fr = frames.synthetic_frame(frame)
    if W == H:
        return oracle.Net(blob).forward(oracle.preprocess(fr, W))
    return TorchNet(blob).forward(rect_ref.preprocess(fr, W, H)).numpy()


def decode(head, W, H, nc, nk, **kw):
    return oracle.decode_nms(head, W, nc, nk, **kw) if W == H else rect_ref.decode_nms(head, W, H, nc, nk, **kw)


@pytest.fixture(scope="module")
def zero_heads(blob):
    """(W, H) -> oracle head of the all-zeroed blob (ladder classes, wide boxes, quad keypoints), computed once."""
    cls, box, kpt = dc.ladder_bias(14), dc.WIDE_BOXES, dc.quad_kpt_bias(8)
    b = dc.craft(blob, cls=("bias", cls), box=("bias", box), kpt=("bias", kpt))
    return {(W, H): oracle_head(b, W, H, 3) for W, H in ((64, 64), (96, 96), (416, 416), (640, 512))}, (cls, box, kpt)


def test_craft_touches_only_the_finals(blob):
    b = dc.craft(blob, cls=("bias", dc.ladder_bias(14)), box={1: ("shift", 0.5)}, kpt=("bias", dc.quad_kpt_bias(8)), levels=(1, 2))
    h0, l0 = weights.parse_blob(blob)
    h1, l1 = weights.parse_blob(b)
    assert h0 == h1 and len(l0) == len(l1)
    changed = []
    for (s0, w0, b0), (s1, w1, b1) in zip(l0, l1):
        assert s0 == s1
        if not (np.array_equal(w0, w1) and np.array_equal(b0, b1)):
            changed.append(s0.name)
    assert sorted(changed) == sorted(["model.22.cv3.1.2", "model.22.cv3.2.2", "model.22.cv2.1.2", "model.22.cv4.1.2", "model.22.cv4.2.2"])
    t = {s.name: (w, bb) for s, w, bb in l1}
    o = {s.name: (w, bb) for s, w, bb in l0}
    assert np.array_equal(t["model.22.cv2.1.2"][0], o["model.22.cv2.1.2"][0])
    assert np.array_equal(t["model.22.cv2.1.2"][1], o["model.22.cv2.1.2"][1] + np.float32(0.5))
    assert not t["model.22.cv3.2.2"][0].any() and np.array_equal(t["model.22.cv3.2.2"][1], dc.ladder_bias(14))
    # an int8 blob stays an int8 blob with the same layers
    q = weights.quantize_blob_int8(blob)
    hq, _ = weights.parse_blob(dc.craft(q, cls=("bias", dc.ladder_bias(14))))
    assert hq["dtype"] == weights.DTYPE_INT8 and hq["nc"] == 14 and hq["nk"] == 8


def test_logit_thr_and_bias_vectors():
    assert dc.logit_thr(0.25) == np.float32(oracle.lib().orc_logit_threshold(0.25))
    assert dc.logit_thr(0.5) == 0.0 and dc.logit_thr(0.4) == np.float32(oracle.lib().orc_logit_threshold(0.4))
    lad = dc.ladder_bias(14)
    thr = dc.logit_thr(0.25)
    assert lad[3] == thr and (np.diff(lad[:7]) > 0).all() and (lad[7:] == -20).all()
    assert np.array_equal(np.diff(lad[:7].view(np.int32)), np.full(6, -1))     # negative floats: one ulp up is one bit pattern down
    z = dc.zero_edge_bias(14)
    assert np.signbit(z[0]) and not np.signbit(z[1]) and z[0] == z[1] == 0
    assert z[3].view(np.uint32) == 1 and z[5].view(np.uint32) == 0x00800000 and (z[:6:2] <= 0).all()
    assert list(np.nonzero(z > 0)[0]) == [3, 5]


@pytest.mark.parametrize("W,H", [(64, 64), (96, 96), (416, 416), (640, 512)])
def test_zero_weight_finals_give_the_bias_on_every_anchor(zero_heads, W, H):
    heads, (cls, box, kpt) = zero_heads
    head = heads[(W, H)]
    assert head.shape == (sum(dc.level_sizes(W, H)), 86)
    assert np.array_equal(head, dc.expected_head(W, H, cls, box, kpt))
    assert decode(head, W, H, 14, 8)["n_candidates"] == 3 * head.shape[0]       # the ladder: classes 4, 5, 6; class 3 is ON the threshold


@pytest.mark.parametrize("W,H", [(64, 64), (96, 96), (416, 416), (640, 512)])
@pytest.mark.parametrize("box_bin", [0, 15])
def test_closed_forms_equal_the_oracle(W, H, box_bin):
    """Two classes tied at 1.25 on every anchor: 2 A candidates of one score.  Point-like boxes: the survivors are the head of
    the candidate list.  Wide boxes: count and order (the oracle's survivors follow that order and are boxes of the form)."""
    cls, kpt = dc.two_tied_bias(14), dc.quad_kpt_bias(8)
    head = dc.expected_head(W, H, cls, dc.dfl_bias(box_bin), kpt)
    A = head.shape[0]
    for md, cap in PAIRS:
        cf = dc.closed_form(W, H, cls, box_bin, kpt, 0.25, md, cap)
        exp = decode(head, W, H, 14, 8, max_det=md, pre_nms_cap=cap)
        assert cf["n_candidates"] == exp["n_candidates"] == 2 * A
        assert list(cf["order_anchors"][:4]) == [0, 0, 1, 1] and list(cf["order_classes"][:4]) == [4, 9, 4, 9]
        for i, a in enumerate(exp["anchors"]):          # every survivor carries the closed-form box and keypoints of its anchor
            assert np.array_equal(exp["boxes"][i], cf["all_boxes"][a]) and np.array_equal(exp["kpts"][i], cf["all_kpts"][a])
        pos = {(int(a), int(c)): i for i, (a, c) in enumerate(zip(cf["order_anchors"][:cap], cf["order_classes"][:cap]))}
        where = [pos[(int(a), int(c))] for a, c in zip(exp["anchors"], exp["classes"])]
        assert where == sorted(where)                     # ... in the closed form's order, inside the pre-NMS cut
        if box_bin == 0:
            assert cf["num_dets"] == exp["num_dets"] == min(md, cap, 2 * A)
            for k in ("anchors", "classes", "boxes", "kpts"):
                assert np.array_equal(cf[k], exp[k]), (k, md, cap)
        else:
            assert 0 < exp["num_dets"] <= min(md, cap)
            assert where[:3] != [0, 1, 2]                 # chains: something near the head of the list is suppressed


def test_zero_edge_candidates_are_the_classes_above_zero():
    z = dc.zero_edge_bias(14)
    for W, H in ((64, 64), (416, 416)):
        head = dc.expected_head(W, H, z, dc.POINT_BOXES, dc.quad_kpt_bias(8))
        A = head.shape[0]
        cf = dc.closed_form(W, H, z, 0, dc.quad_kpt_bias(8), 0.5, 256, 8192)
        exp = oracle.decode_nms(head, W, 14, 8, score_thr=0.5, max_det=256, pre_nms_cap=8192)
        assert cf["n_candidates"] == exp["n_candidates"] == 2 * A
        assert set(cf["order_classes"]) == {3, 5} and (cf["order_classes"][:A] == 5).all() and (cf["order_classes"][A:] == 3).all()
        for k in ("anchors", "classes", "boxes", "kpts"):
            assert np.array_equal(cf[k], exp[k]), k


def test_one_level_lit_counts():
    for W in (416, 96):
        for L in range(3):
            cls = {l: (dc.ladder_bias(14) if l == L else dc.dark_bias(14)) for l in range(3)}
            head = dc.expected_head(W, W, cls, dc.WIDE_BOXES, dc.quad_kpt_bias(8))
            exp = oracle.decode_nms(head, W, 14, 8)
            cf = dc.closed_form(W, W, cls, 15, dc.quad_kpt_bias(8))
            base, size = dc.level_bases(W, W)[L], dc.level_sizes(W, W)[L]
            assert exp["n_candidates"] == cf["n_candidates"] == 3 * size
            assert ((exp["anchors"] >= base) & (exp["anchors"] < base + size)).all() and exp["num_dets"] > 0
    assert [b % 32 for b in dc.level_bases(416, 416)[1:]] == [16, 20] and [b % 32 for b in dc.level_bases(96, 96)[1:]] == [16, 20]


def density_counts(blob, W, H, delta, frame):
    """(oracle count, count with the threshold HEAD_TOL higher, HEAD_TOL lower) of the class finals shifted by delta."""
    head = oracle_head(dc.craft(blob, cls=("shift", delta)), W, H, frame)
    cl = head[:, 64:78]
    thr = dc.logit_thr(0.25)
    n = decode(head, W, H, 14, 8)["n_candidates"]
    assert n == int((cl > thr).sum())
    return n, int((cl > thr + HEAD_TOL).sum()), int((cl > thr - HEAD_TOL).sum())


@pytest.mark.parametrize("W,H", list(DENSITY))
def test_density_table_sits_inside_its_bands(blob, capsys, W, H):
    A = sum(dc.level_sizes(W, H))
    table = DENSITY[(W, H)]
    assert 0 < len(table) <= 6                              # engines per net
    hit = set()
    lines = []
    for delta, frs, want in table:
        assert len(frs) == len(want) == len(set(frs)), (delta, frs, want)       # a distinct frame in every slot
        for f, band in zip(frs, want):
            n, n_hi, n_lo = density_counts(blob, W, H, delta, f)
            lo, hi = dc.bands(A, 14)[band]
            lines.append(f"  {W}x{H} delta {delta:+g} frame {f}: oracle {n} candidates (threshold +/- HEAD_TOL: {n_hi} .. {n_lo}), band {band}")
            assert dc.inside_with_margin(n, lo, hi), (delta, f, n, band)
            assert lo <= n_hi <= n_lo <= hi, (delta, f, n_hi, n_lo, band)       # whatever the GPU's head is within HEAD_TOL, its count is in the band
            hit.add(band)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert hit == set(dc.bands(A, 14)), sorted(set(dc.bands(A, 14)) - hit)
    assert sum(len(set(want)) > 1 for _, _, want in table) >= 3       # slots of one batched step in different bands
