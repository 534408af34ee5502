"""Host reference of the pose-ambiguity rule (include/irmv_hip.h, "pose ambiguity"; csrc/pnp_device.hpp pose_cost /
pose_pick_b): float64, operation for operation what the kernels do, so that a decision can be compared bit for bit.

IPPE returns two poses per plate.  A is the one the min-error rule reports (solution 0 unless not err0 <= err1), B the other.
With n_X = column 0 of R_X (the plate normal pointing away from the camera), u the slot's unit up vector and s the class's
expected n . u:

    cost_X = fabs(((R_X[0,0]*u[0] + R_X[1,0]*u[1]) + R_X[2,0]*u[2]) - s)
    report B  iff  mode == PRIOR  and  errB <= ratio * errA  and  costB < costA

Any NaN makes a comparison false: A stays.
"""
from __future__ import annotations

import math

import numpy as np

MIN_ERR, PRIOR = 0, 1
NORMAL_UP_ROBOT = -0.25881904510252074    # -sin 15 deg: a plate whose outward normal points 15 degrees upward
NORMAL_UP_OUTPOST = 0.25881904510252074
DEFAULT_RATIO = 8.0
DEFAULT_UP = (0.0, -1.0, 0.0)             # a level camera: image y points down


def normalise_up(v) -> np.ndarray:
    """irmv_engine_set_up's normalisation: v / sqrt((x*x + y*y) + z*z); ValueError for what it refuses (a zero, non-finite or
    NaN vector, or one whose squared length overflows)."""
    x, y, z = (float(c) for c in np.asarray(v, np.float64).reshape(3))
    n = math.sqrt((x * x + y * y) + z * z) if all(math.isfinite(c) for c in (x, y, z)) else math.nan
    if not (n > 0.0 and n < math.inf):
        raise ValueError("up must be finite and non-zero")
    return np.array([x / n, y / n, z / n], np.float64)


def cost(R, u, s) -> float:
    """|n . u - s| in the kernels' association order; R is a 3 x 3 rotation (model -> camera)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    u0, u1, u2 = (float(c) for c in np.asarray(u, np.float64).reshape(3))
    return abs(((float(R[0, 0]) * u0 + float(R[1, 0]) * u1) + float(R[2, 0]) * u2) - float(s))


def select(RA, errA, RB, errB, u, s, ratio=DEFAULT_RATIO, mode=PRIOR) -> bool:
    """True iff the rule reports B (irmv_pose_alt.state == 2)."""
    if int(mode) != PRIOR:
        return False
    errA, errB, ratio = float(errA), float(errB), float(ratio)
    with np.errstate(all="ignore"):
        bound = float(np.float64(ratio) * np.float64(errA))      # (inf * 0 = NaN, quietly: the comparison is then false)
    return bool(errB <= bound and cost(RB, u, s) < cost(RA, u, s))
