"""Class counts other than 14: the blobs, heads, bias vectors and policies of tests/test_class_counts.py (CPU) and
tests/test_gpu_class_counts.py (GPU).

irmv_engine_create accepts a model with 1 .. 16 classes.  The class count sits in the 16-row pad of the class final, in the
`class < nc` mask of the three candidate producers (a lane of a quad owns classes 4q .. 4q + 3), in the key ids
(anchor * nc + class), in the key list's capacity (A * nc), in nms_pnp_kernel's id / nc, id % nc and its per-class
ballots, prefix sum and walking waves, and in the +inf tail of the class policy table.  NCS are the counts at which that
code changes behaviour:

    1    lane 0 of a quad owns one live class, lanes 1 .. 3 none; id % 1 == 0; one walking wave; 15 padded rows; A * nc = A
    4    exactly one lane fully live, three fully masked
    5    one class past a lane boundary
    13   the other side of 14: lane 3 holds one live class
    16   no padded row, no masked class, no +inf tail; classes 14 and 15 exist

nk = 8 everywhere, nk = 0 at nc 1 and 16 (the shortest and the longest head record).

Test infrastructure only; never imported by the product package.
"""
from __future__ import annotations

import functools

import numpy as np

import detect_craft as dc
from irmv_detection_amd import class_policy, weights

NCS = (1, 4, 5, 13, 16)
PAIRS = tuple((nc, 8) for nc in NCS) + ((1, 0), (16, 0))      # (nc, nk)
A640 = 8400
DENSITY_T = (300, 770, 3000, 20000)      # expected candidates of a density head: hot = T / (A nc)


def pair_id(p) -> str:
    return f"nc{p[0]}-nk{p[1]}"


@functools.lru_cache(maxsize=None)
def blob(nc: int, nk: int = 8) -> bytes:
    """The seed-0 synthetic model with nc classes and nk keypoint channels."""
    return weights.synthetic_blob(0, nc=nc, nk=nk)


# ---- heads -----------------------------------------------------------------------------------------------------------
def random_head(rng, A: int, nc: int, nk: int, hot: float) -> np.ndarray:
    """tests/test_oracle_post.py::_random_head: DFL logits with a decaying mean, class logits N(-6, 1) with a fraction `hot`
    of the pairs drawn from U(-1, 4), keypoints around 0.25."""
    head = np.zeros((A, 64 + nc + nk), np.float32)
    head[:, :64] = rng.standard_normal((A, 64)) - 0.4 * (np.arange(64) % 16)
    cls = rng.standard_normal((A, nc)) - 6.0
    mask = rng.random((A, nc)) < hot
    cls[mask] = rng.uniform(-1.0, 4.0, mask.sum())
    head[:, 64:64 + nc] = cls
    head[:, 64 + nc:] = 0.25 + 0.3 * rng.standard_normal((A, nk))
    return head


def density_ts(nc: int, A: int = A640):
    """The T of DENSITY_T a model of nc classes can hold: 1.25 T pairs must exist."""
    return tuple(T for T in DENSITY_T if 1.25 * T <= A * nc)


def density_head(nc: int, nk: int, T: int, seed: int, A: int = A640) -> np.ndarray:
    return random_head(np.random.default_rng(seed), A, nc, nk, T / (A * nc))


def empty_head(nc: int, nk: int, A: int = A640) -> np.ndarray:
    """All nc classes at -20: no candidate -- unless a producer reads the record's class slots nc .. 15."""
    h = random_head(np.random.default_rng(5), A, nc, nk, 0.0)
    h[:, 64:64 + nc] = dc.DARK
    return h


def all_pairs_head(nc: int, nk: int, A: int = A640) -> np.ndarray:
    """Every (anchor, class) pair at 3.0: A * nc tied candidates, exactly the key list's capacity."""
    h = np.zeros((A, 64 + nc + nk), np.float32)
    h[:, 64:64 + nc] = 3.0
    return h


def tie_heads(nc: int, nk: int, A: int = A640) -> dict:
    """Tied scores on neighbouring stride-8 anchors with wide, overlapping boxes: the order is anchor, then class.
    "first and last class": classes 0 and nc - 1 tied on the same 300 anchors (nc = 1: class 0 alone), and class nc - 1 alone
    on the last anchor.  "two classes per anchor": test_gpu_engine._class_walk_heads()["all scores equal, two classes per
    anchor"] with its classes 4 and 9 taken mod nc."""
    rng = np.random.default_rng(404 + nc)
    base = np.zeros((A, 64 + nc + nk), np.float32)
    base[:, :64] = 0.05 * rng.standard_normal((A, 64))
    base[:, 64:64 + nc] = dc.DARK
    base[:, 64 + nc:] = 0.25 + 0.3 * rng.standard_normal((A, nk))
    ends = base.copy()
    ends[:300, 64 + 0] = 1.25
    ends[:300, 64 + nc - 1] = 1.25
    ends[A - 1, 64 + nc - 1] = 1.25
    two = base.copy()
    two[:300, 64 + 4 % nc] = 1.25
    two[100:200, 64 + 9 % nc] = 1.25
    return {"first and last class": ends, "two classes per anchor": two}


# ---- bias vectors of crafted class finals ----------------------------------------------------------------------------
def edge_bias(nc: int, score_thr: float = 0.25) -> np.ndarray:
    """Class nc - 1 one ulp above the logit threshold, class 0 exactly on it (no candidate; nc >= 2), class nc - 2 one ulp
    below (nc >= 3), the rest dark: one candidate per anchor, of the LAST live class."""
    thr = dc.logit_thr(score_thr)
    v = np.full(nc, dc.DARK, np.float32)
    if nc >= 3:
        v[nc - 2] = dc.nextafter_k(thr, -1)
    if nc >= 2:
        v[0] = thr
    v[nc - 1] = dc.nextafter_k(thr, 1)
    return v


def all_lit_bias(nc: int) -> np.ndarray:
    return np.full(nc, np.float32(1.25), np.float32)


# ---- class policies ----------------------------------------------------------------------------------------------------
ABOVE_NC_THR = np.float32(0.05)      # entries at and above nc: below every live threshold, so a minimum over all 16 would show


def last_off_policy(nc: int) -> dict:
    """A threshold of its own per class (0.10, 0.14, ...: all below sigmoid(1.25) = 0.78), class nc - 1 off."""
    thr = np.full(16, ABOVE_NC_THR, np.float32)
    thr[:nc] = (0.1 + 0.04 * np.arange(nc)).astype(np.float32)
    thr[nc - 1] = 1.0
    return class_policy.policy(thr)


def only_last_policy(nc: int) -> dict:
    thr = np.full(16, ABOVE_NC_THR, np.float32)
    thr[:nc] = 1.0
    thr[nc - 1] = 0.3
    return class_policy.policy(thr)
