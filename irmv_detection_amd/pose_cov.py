"""Host reference of the pose uncertainty (include/irmv_hip.h, "pose uncertainty"; csrc/k_posecov.hip, csrc/engine_posecov.cpp):
float64, operation for operation what the kernel does.  Python floats only -- no BLAS, no fused multiply-add, every division
a division --, so that every number can be compared with the device's bit for bit.

The model is the first-order (Gauss-Newton) covariance of a pose under independent corner noise of sigma_px pixels:

    corners      (nx_i, ny_i) = undistort4 of the record's four points (yaw_solve.undistort4)
    object       P_i = (0, cX_i, cY_i), cX = (hy, hy, -hy, -hy), cY = (-hz, hz, hz, -hz): LB, LT, RT, RB of the plate
    rotation     R = rodrigues(rvec) below -- sin and cos as two stated series, because no libm is the same on host and device
    projection   a_i = R P_i,  X_i = a_i + t,  x_i = X_i.x / X_i.z,  y_i = X_i.y / X_i.z
    residuals    r_2i = ((x_i - nx_i) fx) / sigma_px,  r_2i+1 = ((y_i - ny_i) fy) / sigma_px
                 (a pixel residual that ignores the distortion's own Jacobian)
    perturbation R <- exp([w]x) R, t <- t + tau, parameters (w_x, w_y, w_z, tau_x, tau_y, tau_z) in the camera frame:
                 dX_i/dw = -[a_i]x, dX_i/dtau = I
    Jacobian     row 2i:   g = (sx / Z, 0, -(x (sx / Z))),  sx = fx / sigma_px
                 row 2i+1: g = (0, sy / Z, -(y (sy / Z))),  sy = fy / sigma_px
                 J = (g2 a1 - g1 a2,  g0 a2 - g2 a0,  g1 a0 - g0 a1,  g0,  g1,  g2)
    A = J^T J    each of the 21 entries summed over the eight rows in ascending row order
    Cholesky     A = L L^T, column by column; a pivot p with not p > 0 refuses
    Sigma        column c of A^-1 by L y = e_c, then L^T x = y; cov[(i, j)], i <= j, is entry i of column j
    chi2         the eight r^2 summed in ascending order
    sigma_range  sqrt(d^T Sigma_tautau d), d = t / |t|

The yaw block has the parameters (psi, tau): every model axis rotates about the unit up vector u, dX_i/dpsi = u x a_i, so
its Jacobian's first column is (J_w0 u0 + J_w1 u1) + J_w2 u2 of the rows above, evaluated at the constrained pose.
"""
from __future__ import annotations

import math

import numpy as np

from . import yaw_solve

HALF_Y, HALF_Z = yaw_solve.HALF_Y, yaw_solve.HALF_Z
DEFAULT_SIGMA_PX = 1.0
SIGMA_PX_MAX = 64.0
TWO_PI = 6.283185307179586     # the double nearest 2 pi
SERIES_TERMS = 16              # of both series; the reduced angle is in [-pi, pi]
N_COV, N_YAW = 21, 10


def sin_vers(th):
    """(sin th, 1 - cos th) of th >= 0: the angle reduced by the nearest multiple of 2 pi, then the series of sin(a) / a and
    (1 - cos a) / a^2 in a^2 as nested divisions by the integers (2k)(2k + 1) and (2k + 1)(2k + 2)."""
    k = float(np.rint(th / TWO_PI))
    a = th - k * TWO_PI
    x = a * a
    s = 1.0
    c = 1.0
    for j in range(SERIES_TERMS - 1, 0, -1):
        s = 1.0 - (x / float((2 * j) * (2 * j + 1))) * s
        c = 1.0 - (x / float((2 * j + 1) * (2 * j + 2))) * c
    return a * s, x * (0.5 * c)


def rodrigues(rvec):
    """rvec -> R as nine floats, row-major (model -> camera)."""
    r0, r1, r2 = (float(v) for v in rvec)
    th = math.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
    sn, vc = sin_vers(th)
    den = th if th > 0.0 else 1.0
    n0, n1, n2 = r0 / den, r1 / den, r2 / den
    d = 1.0 - vc
    return [d + vc * (n0 * n0), vc * (n0 * n1) - sn * n2, vc * (n0 * n2) + sn * n1,
            vc * (n0 * n1) + sn * n2, d + vc * (n1 * n1), vc * (n1 * n2) - sn * n0,
            vc * (n0 * n2) - sn * n1, vc * (n1 * n2) + sn * n0, d + vc * (n2 * n2)]


def _finite(v):
    return abs(v) < math.inf      # False for a NaN too


def jacobian(R, t, nxy, size, fx, fy, sigma_px):
    """-> (J as 8 rows of 6, r as 8 floats), or None where a corner has depth <= 0 (or NaN)."""
    hy, hz = HALF_Y[size], HALF_Z[size]
    cX, cY = (hy, hy, -hy, -hy), (-hz, hz, hz, -hz)
    sx, sy = fx / sigma_px, fy / sigma_px
    J, r = [], []
    for i in range(4):
        a0 = R[1] * cX[i] + R[2] * cY[i]
        a1 = R[4] * cX[i] + R[5] * cY[i]
        a2 = R[7] * cX[i] + R[8] * cY[i]
        X, Y, Z = a0 + t[0], a1 + t[1], a2 + t[2]
        if not Z > 0.0:
            return None
        x, y = X / Z, Y / Z
        r += [((x - nxy[2 * i]) * fx) / sigma_px, ((y - nxy[2 * i + 1]) * fy) / sigma_px]
        gx0 = sx / Z
        gy1 = sy / Z
        for g0, g1, g2 in ((gx0, 0.0, -(x * gx0)), (0.0, gy1, -(y * gy1))):
            J.append([g2 * a1 - g1 * a2, g0 * a2 - g2 * a0, g1 * a0 - g0 * a1, g0, g1, g2])
    return J, r


def yaw_jacobian(J, u):
    """The 8 x 4 Jacobian of (psi, tau) from the 8 x 6 one at the constrained pose."""
    return [[(row[0] * u[0] + row[1] * u[1]) + row[2] * u[2], row[3], row[4], row[5]] for row in J]


def normal_matrix(J, n):
    """A = J^T J, upper triangle row-major, every entry summed over the rows in ascending order."""
    A = []
    for i in range(n):
        for j in range(i, n):
            s = 0.0
            for row in J:
                s = s + row[i] * row[j]
            A.append(s)
    return A


def tri(i, j, n):
    """Index of (i, j), i <= j, in an upper triangle stored row-major."""
    return i * n - (i * (i - 1)) // 2 + (j - i)


def cholesky_inverse(A, n):
    """A (upper triangle, row-major) -> the upper triangle of its inverse, or None where a pivot is not > 0."""
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        p = A[tri(j, j, n)]
        for k in range(j):
            p = p - L[j][k] * L[j][k]
        if not p > 0.0:
            return None
        L[j][j] = math.sqrt(p)
        for i in range(j + 1, n):
            s = A[tri(j, i, n)]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    cols = []
    for c in range(n):
        y = [0.0] * n
        for k in range(n):
            s = 1.0 if k == c else 0.0
            for m in range(k):
                s = s - L[k][m] * y[m]
            y[k] = s / L[k][k]
        x = [0.0] * n
        for k in range(n - 1, -1, -1):
            s = y[k]
            for m in range(k + 1, n):
                s = s - L[m][k] * x[m]
            x[k] = s / L[k][k]
        cols.append(x)
    return [cols[j][i] for i in range(n) for j in range(i, n)]


def _chi2(r):
    s = 0.0
    for v in r:
        s = s + v * v
    return s


def zero_record(state=0):
    return dict(cov=[0.0] * N_COV, chi2=0.0, sigma_range=0.0, yaw_cov=[0.0] * N_YAW, yaw_chi2=0.0, sigma_yaw=0.0, state=state,
                yaw_state=0)


def unit(up):
    """An up vector normalised as the library's setters do."""
    u0, u1, u2 = (float(v) for v in up)
    ln = math.sqrt((u0 * u0 + u1 * u1) + u2 * u2)
    return (u0 / ln, u1 / ln, u2 / ln)


def pose_cov(cam, pts, size, rvec, tvec, sigma_px=DEFAULT_SIGMA_PX, *, yaw=None, nxy=None):
    """One record.  cam = yaw_solve.camera_of(K, D); pts: float32 pixels LB, LT, RT, RB; yaw: None or (rvec, tvec, u) of the
    constrained pose with the UNIT up vector u.  nxy (tests): the eight normalised coordinates in place of undistort4.
    -> dict(cov[21], chi2, sigma_range, yaw_cov[10], yaw_chi2, sigma_yaw, state, yaw_state)."""
    out = zero_record(-1)
    pts = np.asarray(pts if nxy is None else np.zeros(8), np.float32).reshape(8)
    rvec, tvec = [float(v) for v in rvec], [float(v) for v in tvec]
    if not all(abs(float(v)) < 16777216.0 for v in pts) or not all(abs(v) < 1e300 for v in rvec + tvec):
        return out
    fx, fy = float(cam[0]), float(cam[1])
    sigma_px = float(sigma_px)
    with np.errstate(all="ignore"):
        nxy = yaw_solve.undistort4(cam, pts) if nxy is None else [float(v) for v in nxy]
    try:
        jr = jacobian(rodrigues(rvec), tvec, nxy, size, fx, fy, sigma_px)
        if jr is None:
            return out
        J, r = jr
        cov = cholesky_inverse(normal_matrix(J, 6), 6)
        if cov is None:
            return out
        chi2 = _chi2(r)
        t0, t1, t2 = tvec
        ln = math.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
        d = (t0 / ln, t1 / ln, t2 / ln)
        S = [[cov[tri(min(i, j), max(i, j), 6)] for j in range(3, 6)] for i in range(3, 6)]
        q = 0.0
        for i in range(3):
            q = q + d[i] * ((S[i][0] * d[0] + S[i][1] * d[1]) + S[i][2] * d[2])
        sigma_range = math.sqrt(q) if q >= 0.0 else math.nan
    except (ZeroDivisionError, OverflowError, ValueError):
        return out
    if not all(_finite(v) for v in cov + [chi2, sigma_range]):
        return out
    out.update(cov=cov, chi2=chi2, sigma_range=sigma_range, state=1)
    if yaw is None:
        return out
    out["yaw_state"] = -1
    yr, yt, u = ([float(v) for v in a] for a in yaw)
    if not all(abs(v) < 1e300 for v in yr + yt + u):
        return out
    try:
        jr = jacobian(rodrigues(yr), yt, nxy, size, fx, fy, sigma_px)
        if jr is None:
            return out
        J, r = jr
        ycov = cholesky_inverse(normal_matrix(yaw_jacobian(J, u), 4), 4)
        if ycov is None:
            return out
        ychi2 = _chi2(r)
        sigma_yaw = math.sqrt(ycov[0]) if ycov[0] >= 0.0 else math.nan
    except (ZeroDivisionError, OverflowError, ValueError):
        return out
    if not all(_finite(v) for v in ycov + [ychi2, sigma_yaw]):
        return out
    out.update(yaw_cov=ycov, yaw_chi2=ychi2, sigma_yaw=sigma_yaw, yaw_state=1)
    return out


def full(cov, n=6):
    """The upper triangle as a symmetric n x n array."""
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            M[i, j] = M[j, i] = cov[tri(i, j, n)]
    return M


# geometry_msgs/PoseWithCovariance orders (x, y, z, rot_x, rot_y, rot_z): entry (a, b) of its 6 x 6 is entry (ROS_ORDER[a],
# ROS_ORDER[b]) of this one
ROS_ORDER = (3, 4, 5, 0, 1, 2)


def ros_covariance(cov):
    """cov[21] -> the 36 row-major entries of a geometry_msgs/PoseWithCovariance (translation first), in the camera frame."""
    M = full(cov)
    return [float(M[ROS_ORDER[a], ROS_ORDER[b]]) for a in range(6) for b in range(6)]


def record_of(rec):
    """A capi.PoseCov structure -> the dict pose_cov() returns."""
    return dict(cov=list(rec.cov), chi2=rec.chi2, sigma_range=rec.sigma_range, yaw_cov=list(rec.yaw_cov), yaw_chi2=rec.yaw_chi2,
                sigma_yaw=rec.sigma_yaw, state=int(rec.state), yaw_state=int(rec.yaw_state))
