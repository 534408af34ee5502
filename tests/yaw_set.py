"""What the constrained-pose tests share (tests/test_yaw_solve.py, tests/test_gpu_yaw_solve.py): the reference camera, the host
reference on the lean-back set (computed once, never changed) and the yaw-error statistics.  No GPU here."""
import functools

import numpy as np

import pnp_ref as P
import pose_prior_set as L
from irmv_detection_amd import yaw_solve as Y

_, K, D = P.CAMERAS[L.CAM]
CAM = Y.camera_of(K, D)


def tilt_up(u, deg):
    """u turned by `deg` degrees about the optical axis' horizontal direction h1: an attitude error of the gimbal."""
    h1, _ = Y.basis(u)
    k = np.array(h1)
    a = np.radians(deg)
    u = np.asarray(u, np.float64)
    v = u * np.cos(a) + np.cross(k, u) * np.sin(a) + k * (k @ u) * (1 - np.cos(a))
    return v / np.linalg.norm(v)


@functools.lru_cache(None)
def reference_set(tilt_deg=0.0):
    """The reference's solve of every case of the lean-back set, with its up vector turned by tilt_deg -> tuple of dicts."""
    return tuple(Y.solve(CAM, c["pts"], L.SIZE, c["u"] if tilt_deg == 0.0 else tilt_up(c["u"], tilt_deg), L.S) for c in L.lean_back_set())


def stats(errors):
    e = np.asarray(errors, np.float64)
    return dict(median=float(np.median(e)), p90=float(np.percentile(e, 90)), rms=float(np.sqrt((e * e).mean())),
                over10=int((e > 10).sum()), over20=int((e > 20).sum()))


def set_errors(tilt_deg=0.0):
    """-> (min-error, prior, constrained) yaw errors in degrees over the lean-back set, against the generating poses.  The
    first two are the mpmath reference's IPPE solutions under the two rules (the prior with the true up vector)."""
    cases = L.lean_back_set()
    e_min = [Y.yaw_error(np.array(c["ref"]["R"][0], np.float64), c["R"], c["u"]) for c in cases]
    e_pri = [Y.yaw_error(np.array(c["ref"]["R"][1 if c["pick"] else 0], np.float64), c["R"], c["u"]) for c in cases]
    e_yaw = [Y.yaw_error(r["R"], c["R"], c["u"]) if r["state"] == 1 else 180.0 for c, r in zip(cases, reference_set(tilt_deg))]
    return e_min, e_pri, e_yaw
