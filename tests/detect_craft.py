"""Crafted Detect finals: weight blobs whose head is known before a step runs.

The final 1x1 of every Detect branch (model.22.cv{2,3,4}.{level}.2) computes w . x + b in fp32.  With its weights zeroed
the branch's columns of the head equal its bias, as values, on every anchor of the level (a -0.0 bias may come back as
+0.0: the accumulator it is added to is +0.0) -- whatever the frame, whatever the backbone computes.  craft() rewrites
only those layers of a blob, so a whole step -- candidate emission in the class carriers' epilogues, the gated row stores
of the box carriers and the keypoint launch, the launch order of the sparse head plan -- runs on a head chosen by the
test: thousands of tied scores, logits exactly on the threshold, levels fully lit or fully dark.

closed_form() states, independently of oracle/orc_post.c, what decode / NMS must return for a blob with all three finals
zeroed: the candidate count and order, and for point-like boxes (nothing overlaps, nothing is suppressed) the survivors
with their boxes and keypoints.  tests/test_detect_craft.py holds both against the CPU oracle.

Test infrastructure only; never imported by the product package.
"""
from __future__ import annotations

import numpy as np

from irmv_detection_amd import weights

STRIDES = (8, 16, 32)
REG_MAX = 16
BRANCH = {"cv3": "cls", "cv2": "box", "cv4": "kpt"}
SUBNORMAL = np.float32(1.401298464324817e-45)     # the smallest positive fp32 subnormal, 2^-149
FLT_MIN = np.float32(1.1754943508222875e-38)      # the smallest positive fp32 normal, 2^-126
DARK = np.float32(-20.0)                          # a class logit no threshold here reaches
OFF_BIN = np.float32(-100.0)                      # a DFL logit whose bin carries no mass: exp(-100) rounds away against 1


# ---- blobs -----------------------------------------------------------------------------------------------------------
def _treatment(spec, level):
    if isinstance(spec, dict):
        spec = spec.get(level)
    return spec


def craft(blob: bytes, cls=None, box=None, kpt=None, levels=(0, 1, 2)) -> bytes:
    """A copy of `blob` with the finals model.22.cv{3,2,4}.{i}.2 of `levels` rewritten; every other layer, nc, nk, the
    backbone and the weight dtype are kept.  cls / box / kpt: None (keep), ("bias", vector): zero weights and that bias,
    ("shift", delta): the weights kept, delta added to every bias -- or a dict level -> one of these."""
    hdr, layers = weights.parse_blob(blob)
    spec = {"cls": cls, "box": box, "kpt": kpt}
    specs, tensors = [], []
    for sp, w, b in layers:
        p = sp.name.split(".")
        w, b = w.copy(), b.copy()
        if len(p) == 5 and p[0] == "model" and p[1] == "22" and p[2] in BRANCH and p[4] == "2" and int(p[3]) in levels:
            t = _treatment(spec[BRANCH[p[2]]], int(p[3]))
            if t is not None:
                kind, v = t
                if kind == "bias":
                    v = np.asarray(v, np.float32)
                    assert v.shape == b.shape, (sp.name, v.shape, b.shape)
                    w[:] = 0
                    b = v.copy()
                elif kind == "shift":
                    b = (b + np.float32(v)).astype(np.float32)
                else:
                    raise ValueError(kind)
        specs.append(sp)
        tensors.append((w, b))
    build = weights.build_blob_int8 if hdr["dtype"] == weights.DTYPE_INT8 else weights.build_blob
    return build(specs, tensors, hdr["nc"], hdr["nk"], hdr["backbone"])


# ---- bias vectors ----------------------------------------------------------------------------------------------------
def logit_thr(score_thr: float) -> np.float32:
    """The engine's threshold on the logit: float32(log(t / (1 - t))) evaluated in float64 on the float32 score threshold."""
    t = np.float64(np.float32(score_thr))
    return np.float32(np.log(t / (1.0 - t)))


def nextafter_k(x, k: int) -> np.float32:
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def ladder_bias(nc: int, score_thr: float = 0.25) -> np.ndarray:
    """Classes 0 .. 6 at nextafter^k(logit_thr), k = -3 .. +3 -- class 3 exactly ON the threshold, three classes one, two
    and three ulps above it --, every other class dark.  3 candidates per anchor."""
    assert nc >= 7
    v = np.full(nc, DARK, np.float32)
    for c, k in enumerate(range(-3, 4)):
        v[c] = nextafter_k(logit_thr(score_thr), k)
    return v


def zero_edge_bias(nc: int) -> np.ndarray:
    """For score_thr 0.5 (logit_thr exactly 0): -0.0, +0.0, -/+ the smallest subnormal, -/+ FLT_MIN, the rest dark.  The
    candidates are the classes whose value is > 0: 3 and 5."""
    assert nc >= 6 and logit_thr(0.5) == 0.0
    v = np.full(nc, DARK, np.float32)
    v[:6] = [-0.0, 0.0, -SUBNORMAL, SUBNORMAL, -FLT_MIN, FLT_MIN]
    return v


def two_tied_bias(nc: int, classes=(4, 9), value: float = 1.25) -> np.ndarray:
    v = np.full(nc, DARK, np.float32)
    v[list(classes)] = np.float32(value)
    return v


def dark_bias(nc: int, value: float = -30.0) -> np.ndarray:
    return np.full(nc, np.float32(value), np.float32)


def dfl_bias(hot_bin: int) -> np.ndarray:
    """All DFL mass of all four sides on one bin: the hot bin at 0, the others at -100 (their exp is below half an ulp of
    the sum, and of 15 times the hot bin's).  Bin 0: point-like boxes, nothing overlaps; bin 15: every side 15 strides
    long, neighbouring anchors overlap and suppress in long chains."""
    v = np.full(4 * REG_MAX, OFF_BIN, np.float32)
    v[hot_bin::REG_MAX] = 0.0
    return v


POINT_BOXES, WIDE_BOXES = dfl_bias(0), dfl_bias(REG_MAX - 1)


def quad_kpt_bias(nk: int = 8) -> np.ndarray:
    """Constant keypoint biases: an armor-like quad around the anchor (weights.KPT_BASE: lb, lt, rt, rb)."""
    base = np.array(weights.KPT_BASE, np.float32).reshape(-1)[:nk]
    return (np.float32(0.25) + base / np.float32(2.0)).astype(np.float32)


# ---- closed forms ----------------------------------------------------------------------------------------------------
def anchor_table(W: int, H: int):
    """Per anchor of a W x H net, in head order: column ix, row iy, stride, level."""
    ix, iy, st, lv = [], [], [], []
    for l, s in enumerate(STRIDES):
        w, h = W // s, H // s
        ix.append(np.tile(np.arange(w), h))
        iy.append(np.repeat(np.arange(h), w))
        st.append(np.full(w * h, s))
        lv.append(np.full(w * h, l))
    return tuple(np.concatenate(v).astype(np.int64) for v in (ix, iy, st, lv))


def level_sizes(W: int, H: int):
    return [(W // s) * (H // s) for s in STRIDES]


def level_bases(W: int, H: int):
    return [int(v) for v in np.concatenate([[0], np.cumsum(level_sizes(W, H))[:-1]])]


def _per_level(v, nlev=3):
    return [np.asarray(v[l], np.float32) for l in range(nlev)] if isinstance(v, dict) else [np.asarray(v, np.float32)] * nlev


def expected_head(W: int, H: int, cls, box, kpt) -> np.ndarray:
    """The head of a blob with all three finals zeroed: every row of a level is [box bias | class bias | keypoint bias]
    (each a vector or a dict level -> vector)."""
    _, _, _, lv = anchor_table(W, H)
    rows = [np.concatenate([b, c, k]) for b, c, k in zip(_per_level(box), _per_level(cls), _per_level(kpt))]
    return np.stack(rows)[lv].astype(np.float32)


def closed_form(W: int, H: int, cls, box_bin: int, kpt, score_thr: float = 0.25, max_det: int = 100,
                pre_nms_cap: int = 4096) -> dict:
    """What decode / NMS returns on expected_head(W, H, cls, dfl_bias(box_bin), kpt), from the anchor grid and the biases:
    n_candidates; the sorted candidate list (order_anchors, order_classes: score descending, then anchor ascending, then
    class ascending); every candidate's box, and keypoints (2 b + ix) s in fp32.  For point-like boxes (box_bin 0) also
    the survivors: the first min(max_det, pre_nms_cap, n) of the list (num_dets, anchors, classes, boxes, kpts)."""
    ix, iy, st, lv = anchor_table(W, H)
    thr = logit_thr(score_thr)
    cl = np.stack(_per_level(cls))[lv]                                  # [A, nc]
    a_idx, c_idx = np.nonzero(cl > thr)
    val = cl[a_idx, c_idx]
    order = np.lexsort((c_idx, a_idx, -val.astype(np.float64)))         # last key first: score desc, anchor, class
    oa, oc = a_idx[order], c_idx[order]
    s = st.astype(np.float32)
    cx, cy = ix.astype(np.float32) + np.float32(0.5), iy.astype(np.float32) + np.float32(0.5)
    d = np.float32(box_bin)
    boxes = np.stack([(cx - d) * s, (cy - d) * s, (cx + d) * s, (cy + d) * s], 1).astype(np.float32)
    kp = np.stack(_per_level(kpt))[lv]                                  # [A, nk]
    grid = np.stack([ix, iy], 1).astype(np.float32)
    grid = np.tile(grid, (1, kp.shape[1] // 2))
    kpts = ((np.float32(2.0) * kp + grid) * s[:, None]).astype(np.float32)
    out = dict(n_candidates=len(oa), order_anchors=oa.astype(np.int32), order_classes=oc.astype(np.int32),
               all_boxes=boxes, all_kpts=kpts)
    if box_bin == 0:
        n = min(max_det, pre_nms_cap, len(oa))
        out.update(num_dets=n, anchors=oa[:n].astype(np.int32), classes=oc[:n].astype(np.int32), boxes=boxes[oa[:n]],
                   kpts=kpts[oa[:n]])
    return out


def to_source(kpts_net: np.ndarray, src_size, W: int, H: int) -> np.ndarray:
    """Net-input keypoints -> source pixels of a stretch-resize engine: x * (float32(sw) / float32(W)), in fp32."""
    k = np.asarray(kpts_net, np.float32).copy()
    k[:, 0::2] = k[:, 0::2] * (np.float32(src_size[0]) / np.float32(W))
    k[:, 1::2] = k[:, 1::2] * (np.float32(src_size[1]) / np.float32(H))
    return k


# ---- decoy -----------------------------------------------------------------------------------------------------------
def decoy_head(A: int, no: int, nc: int, seed: int) -> np.ndarray:
    """A head no step produces: box and keypoint columns around +/- 1000 (a DFL logit or a keypoint offset never gets
    there), class columns dark.  A row a step fails to store is certainly wrong."""
    rng = np.random.default_rng(seed)
    h = (1000.0 + 50.0 * rng.standard_normal((A, no))).astype(np.float32)
    h[:, 1::2] *= -1.0
    h[:, 64:64 + nc] = -50.0 - rng.random((A, nc)).astype(np.float32)
    return h


# ---- density bands ---------------------------------------------------------------------------------------------------
def bands(A: int, nc: int):
    """name -> (lo, hi) inclusive candidate-count bands the density cases must hit."""
    return {"0": (0, 0), "1-64": (1, 64), "513-1024": (513, 1024), "1025-4096": (1025, 4096), "4097-8192": (4097, 8192),
            ">8192": (8193, A * nc - 1), "all": (A * nc, A * nc)}


def band_of(n: int, A: int, nc: int):
    for name, (lo, hi) in bands(A, nc).items():
        if lo <= n <= hi:
            return name
    return None


def inside_with_margin(n: int, lo: int, hi: int) -> bool:
    """n keeps 20 % of the band's width clear of either edge (a one-value band has no width: n must be it)."""
    m = 0.2 * (hi - lo)
    return lo + m <= n <= hi - m
