"""Host reference of the class policy (irmv_class_policy, include/irmv_hip.h).

A class policy holds one score threshold and one plate model per class.  (anchor, c) is a candidate iff its class logit is
above float32(log(t / (1 - t))), evaluated in float64 on the float32 threshold t of class c; a threshold of 1 or more
switches the class off (+inf).  `table` is irmv_class_policy_table in numpy, `enemy` irmv_class_policy_enemy, and `erase`
states a policy on a head: what decode / NMS at the smallest enabled threshold then returns is what an engine under the
policy must return."""
from __future__ import annotations

import numpy as np

MAX_CLASSES = 16
ARMOR_SMALL, ARMOR_LARGE = 0, 1
DARK = np.float32(-20.0)      # a class logit no threshold of a test reaches (tests/detect_craft.py uses the same value)
BLUE, RED = range(0, 7), range(7, 14)    # ArmorClass B1..BS, R1..RS (include/irmv_detection/armor.hpp)


def _per_class(v, default, dtype):
    a = np.asarray(default if v is None else v, dtype)
    if a.ndim == 0:
        return np.full(MAX_CLASSES, a, dtype)
    if a.ndim != 1 or len(a) > MAX_CLASSES:
        raise ValueError(f"expected a scalar or at most {MAX_CLASSES} per-class values")
    out = np.full(MAX_CLASSES, default, dtype)
    out[:len(a)] = a
    return out


def policy(score_thr=0.25, plate=ARMOR_SMALL) -> dict:
    """A policy as a dict of two arrays of 16: score_thr (float32) and plate (uint8).  Each argument is a scalar or a
    per-class sequence (classes beyond a shorter sequence: 0.25 / SMALL; a model has no such class)."""
    return dict(score_thr=_per_class(score_thr, 0.25, np.float32), plate=_per_class(plate, ARMOR_SMALL, np.uint8))


def uniform(score_thr=0.25, armor_size=ARMOR_SMALL) -> dict:
    """irmv_class_policy_uniform."""
    return policy(float(score_thr), int(armor_size))


def enemy(c: int, score_thr=0.25, armor_size=ARMOR_SMALL) -> dict:
    """irmv_class_policy_enemy: c = 0, the enemy is blue: B1..BS (0..6) on, R1..RS (7..13) off; 1: the reverse; -1: both on."""
    if c not in (-1, 0, 1):
        raise ValueError("enemy colour must be 0 (blue), 1 (red) or -1 (both)")
    p = uniform(score_thr, armor_size)
    if c >= 0:
        p["score_thr"][list(RED if c == 0 else BLUE)] = np.float32(1.0)
    return p


def table(p: dict, nc: int):
    """irmv_class_policy_table: (logit_thr float32[16], min_logit_thr float32).  Raises ValueError where the library
    returns IRMV_ERR_ARG."""
    if not 1 <= nc <= MAX_CLASSES:
        raise ValueError("nc must be 1..16")
    t = np.asarray(p["score_thr"], np.float32)
    pl = np.asarray(p["plate"])
    if t.shape != (MAX_CLASSES,) or pl.shape != (MAX_CLASSES,):
        raise ValueError("a policy holds 16 thresholds and 16 plates")
    if not np.all(t[:nc] > 0):      # (a NaN fails the comparison too)
        raise ValueError("score_thr must be above 0 (>= 1: the class is off)")
    if not np.all((pl[:nc] == ARMOR_SMALL) | (pl[:nc] == ARMOR_LARGE)):
        raise ValueError("plate must be ARMOR_SMALL or ARMOR_LARGE")
    out = np.full(MAX_CLASSES, np.inf, np.float32)
    for c in range(nc):
        if t[c] < 1:
            d = np.float64(t[c])
            out[c] = np.float32(np.log(d / (1.0 - d)))
    return out, np.float32(out.min())


def passes(head: np.ndarray, p: dict, nc: int) -> np.ndarray:
    """bool [A, nc]: the (anchor, class) pairs of a head [A, 64 + nc + nk] that are candidates under the policy."""
    thr, _ = table(p, nc)
    return np.asarray(head, np.float32)[:, 64:64 + nc] > thr[:nc]


def erase(head: np.ndarray, p: dict, nc: int, dark=DARK) -> np.ndarray:
    """A copy of the head with every class logit that fails its own class's threshold set to `dark`.  Decode / NMS of the
    copy at any threshold between `dark` and the smallest enabled one (min_score_thr) is the policy's result."""
    h = np.array(head, np.float32, copy=True)
    cl = h[:, 64:64 + nc]
    cl[~passes(head, p, nc)] = np.float32(dark)
    return h


def min_score_thr(p: dict, nc: int) -> float:
    """The smallest enabled score threshold of the policy (what erase's reference decodes at); None: every class is off."""
    t = np.asarray(p["score_thr"], np.float32)[:nc]
    on = t[t < 1]
    return float(on.min()) if len(on) else None
