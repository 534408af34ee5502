"""Host reference of the constrained pose (include/irmv_hip.h, "constrained pose"; csrc/k_yaw.hip, csrc/engine_yaw.cpp):
float64, operation for operation what the host tables and the kernel do.  Python floats and element-wise arithmetic only --
no BLAS, no fused multiply-add --, so that every number can be compared with the device's.

A plate has one free rotational degree of freedom once the slot's up vector u, the class's tilt s = n . u and the fact that
its long edge is horizontal are used:

    per slot:   g = e_z - (e_z . u) u,  h1 = g / |g|,  h2 = u x h1;   |g|^2 < horizon_min: no basis
    per class:  c = sqrt(1 - s s);   c == 0: no basis
    tau = tan(psi / 2):  d = 1 + tau tau,  cs = (1 - tau tau) / d,  sn = (2 tau) / d
                n = s u + c (cs h1 + sn h2),  y = cs h2 - sn h1,  z = n x y,  R = [n y z]
    translation: the IPPE solver's least-squares translation for R (csrc/pnp_device.hpp ippe_translation)
    q(tau): the sum of the eight squared normalised residuals; +inf for a corner of depth <= 0, for not n . t > 0, for a NaN

The search walks a 64-point grid `rounds` times: tau_k = lo + ((hi - lo) k) / 63, the k of least q (ties: the lower k), then
[max(tau* - step, -tau_max), min(tau* + step, tau_max)] with step = (hi - lo) / 63.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULT_ROUNDS, DEFAULT_TAU_MAX, DEFAULT_HORIZON_MIN = 4, 1.0, 1e-4
LANES = 64
HALF_Y = (135.0 / 2.0 / 1000.0, 225.0 / 2.0 / 1000.0)   # the library's plates: small, large (model y)
HALF_Z = (55.0 / 2.0 / 1000.0, 55.0 / 2.0 / 1000.0)
INF = math.inf


def basis(u, horizon_min=DEFAULT_HORIZON_MIN):
    """The unit up vector u -> (h1, h2) as tuples of floats, or None where the slot has no basis."""
    u0, u1, u2 = (float(c) for c in np.asarray(u, np.float64).reshape(3))
    ezu = u2
    g = (0.0 - ezu * u0, 0.0 - ezu * u1, 1.0 - ezu * u2)
    g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    if not g2 >= horizon_min:
        return None
    ln = math.sqrt(g2)
    h1 = (g[0] / ln, g[1] / ln, g[2] / ln)
    h2 = (u1 * h1[2] - u2 * h1[1], u2 * h1[0] - u0 * h1[2], u0 * h1[1] - u1 * h1[0])
    return h1, h2


def tilt_c(s):
    """c = sqrt(1 - s s); 0.0 or NaN: the class has no basis."""
    v = 1.0 - float(s) * float(s)
    return math.sqrt(v) if v >= 0.0 else math.nan


def rotation(tau, u, h1, h2, s, c):
    """-> (R as a 3 x 3 nested list, rows; columns n, y, z), cs, sn."""
    tt = tau * tau
    d = 1.0 + tt
    cs, sn = (1.0 - tt) / d, (2.0 * tau) / d
    n = [s * u[i] + c * (cs * h1[i] + sn * h2[i]) for i in range(3)]
    y = [cs * h2[i] - sn * h1[i] for i in range(3)]
    z = [n[1] * y[2] - n[2] * y[1], n[2] * y[0] - n[0] * y[2], n[0] * y[1] - n[1] * y[0]]
    return [[n[i], y[i], z[i]] for i in range(3)], cs, sn


def undistort4(cam, pts):
    """csrc/pnp_device.hpp undistort4: float32 pixels [8] -> the eight normalised coordinates.  cam = (fx, fy, cx, cy, k1, k2,
    p1, p2, k3)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (float(v) for v in cam)
    out = []
    for i in range(4):
        x0 = (float(pts[2 * i]) - cx) / fx
        y0 = (float(pts[2 * i + 1]) - cy) / fy
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dx) * icd
            y = (y0 - dy) * icd
        out += [x, y]
    return out


def camera_of(K, D):
    K = np.asarray(K, np.float64).reshape(9)
    D = list(np.asarray(D, np.float64).reshape(-1)) + [0.0] * 5
    return (K[0], K[4], K[2], K[5], D[0], D[1], D[2], D[3], D[4])


def _translation(cX, cY, nxy, Rc):
    """csrc/pnp_device.hpp ippe_translation -> t or None."""
    a02 = a12 = a22 = b0 = b1 = b2 = 0.0
    for i in range(4):
        X, Y, x, y = cX[i], cY[i], nxy[2 * i], nxy[2 * i + 1]
        rx = Rc[0][0] * X + Rc[0][1] * Y
        ry = Rc[1][0] * X + Rc[1][1] * Y
        rz = Rc[2][0] * X + Rc[2][1] * Y
        e1, e2 = x * rz - rx, y * rz - ry
        a02 -= x
        a12 -= y
        a22 += x * x + y * y
        b0 += e1
        b1 += e2
        b2 += -x * e1 - y * e2
    det = 4.0 * (4.0 * a22 - a12 * a12) - a02 * (4.0 * a02)
    if not abs(det) > 1e-300:
        return None
    i00, i01, i02 = 4.0 * a22 - a12 * a12, a02 * a12, -4.0 * a02
    i11, i12, i22 = 4.0 * a22 - a02 * a02, -4.0 * a12, 16.0
    return [(i00 * b0 + i01 * b1 + i02 * b2) / det, (i01 * b0 + i11 * b1 + i12 * b2) / det, (i02 * b0 + i12 * b1 + i22 * b2) / det]


def evaluate(tau, u, h1, h2, s, c, nxy, size):
    """One lane of the kernel (yaw_eval) -> dict(R, t, cs, sn, q).  tau: a float, or an array of them (one per lane): every
    operation is element-wise, so a lane's numbers are the scalar call's."""
    tau = np.asarray(tau, np.float64)
    with np.errstate(all="ignore"):
        R, cs, sn = rotation(tau, u, h1, h2, s, c)
        hy, hz = HALF_Y[size], HALF_Z[size]
        cX, cY = (hy, hy, -hy, -hy), (-hz, hz, hz, -hz)
        Rc = [[R[i][1], R[i][2], R[i][0]] for i in range(3)]       # the solver's canonical frame: columns y, z, n
        t = _translation(cX, cY, nxy, Rc)
        ok = np.ones(tau.shape, bool)
        if t is None:
            ok[...] = False
            t = [np.zeros(tau.shape)] * 3
        q = np.zeros(tau.shape)
        for i in range(4):
            X = Rc[0][0] * cX[i] + Rc[0][1] * cY[i] + t[0]
            Y = Rc[1][0] * cX[i] + Rc[1][1] * cY[i] + t[1]
            Z = Rc[2][0] * cX[i] + Rc[2][1] * cY[i] + t[2]
            ok &= Z > 0.0
            ex, ey = X / Z - nxy[2 * i], Y / Z - nxy[2 * i + 1]
            q = q + (ex * ex + ey * ey)
        nt = (R[0][0] * t[0] + R[1][0] * t[1]) + R[2][0] * t[2]
        ok &= nt > 0.0
        q = np.where(ok & (q < INF), q, INF)
    return dict(R=R, t=t, cs=cs, sn=sn, q=q)


def lane_tau(lo, hi, k):
    return lo + ((hi - lo) * k) / 63.0


def solve(cam, pts, size, u, s, rounds=DEFAULT_ROUNDS, tau_max=DEFAULT_TAU_MAX, horizon_min=DEFAULT_HORIZON_MIN, nxy=None):
    """The kernel's walk on one quad (float32 pixels LB, LT, RT, RB) -> dict(state, tau, cs, sn, err, R (3 x 3 array), t, lane
    (six entries), step (the last round's grid step)).  state 0: a coordinate out of range; -1: refused; 1: solved.
    nxy (tests): the eight normalised coordinates themselves, in place of undistort4(cam, pts)."""
    pts = np.asarray(pts if nxy is None else np.zeros(8), np.float32).reshape(8)
    out = dict(state=0, tau=0.0, cs=0.0, sn=0.0, err=0.0, R=np.zeros((3, 3)), t=np.zeros(3), lane=[0] * 6, step=0.0)
    if not all(abs(float(v)) < 16777216.0 for v in pts):
        return out
    out.update(state=-1, lane=[-1] * 6)
    b = basis(u, horizon_min)
    c = tilt_c(s)
    if b is None or not c > 0.0:
        return out
    u = tuple(float(v) for v in np.asarray(u, np.float64).reshape(3))
    s = float(s)
    h1, h2 = b
    nxy = undistort4(cam, pts) if nxy is None else [float(v) for v in nxy]
    lo, hi, tau, step = -tau_max, tau_max, 0.0, 0.0
    for r in range(rounds):
        qs = evaluate(lane_tau(lo, hi, np.arange(LANES, dtype=np.float64)), u, h1, h2, s, c, nxy, size)["q"]
        k = int(np.argmin(qs))                                   # the first of equal minima: the lower lane
        if r == 0 and not qs[k] < INF:
            return out
        out["lane"][r] = k
        tau = float(lane_tau(lo, hi, float(k)))
        step = (hi - lo) / 63.0
        lo, hi = max(tau - step, -tau_max), min(tau + step, tau_max)
    e = evaluate(tau, u, h1, h2, s, c, nxy, size)
    if not e["q"] < INF:
        return out
    out.update(state=1, tau=tau, cs=float(e["cs"]), sn=float(e["sn"]), err=math.sqrt(float(e["q"]) / 8.0), R=np.array(e["R"], np.float64),
               t=np.array(e["t"], np.float64), step=step)
    return out


def at_tau(cam, pts, size, u, s, tau, horizon_min=DEFAULT_HORIZON_MIN):
    """The model evaluated at a given tau (the device's): dict(R, t, cs, sn, q, err)."""
    h1, h2 = basis(u, horizon_min)
    uu = tuple(float(v) for v in np.asarray(u, np.float64).reshape(3))
    e = evaluate(float(tau), uu, h1, h2, float(s), tilt_c(s), undistort4(cam, np.asarray(pts, np.float32).reshape(8)), size)
    e["err"] = math.sqrt(float(e["q"]) / 8.0)
    e["R"], e["t"] = np.array(e["R"], np.float64), np.array(e["t"], np.float64)
    return e


def yaw_of(R, u, horizon_min=DEFAULT_HORIZON_MIN):
    """The yaw (degrees) of a pose: the angle of its normal (column 0 of R) in the slot's horizontal plane, from h1 towards
    h2.  For a constrained pose this is psi = 2 atan(tau)."""
    h1, h2 = basis(u, horizon_min)
    n = np.asarray(R, np.float64).reshape(3, 3)[:, 0]
    return math.degrees(math.atan2(float(n @ np.array(h2)), float(n @ np.array(h1))))


def yaw_error(R, R_true, u):
    d = yaw_of(R, u) - yaw_of(R_true, u)
    return abs((d + 180.0) % 360.0 - 180.0)
