"""The pose sets of the pose-uncertainty tests (tests/test_pose_cov.py, tests/test_gpu_pose_cov.py) and the checks both share.
No GPU here.

hard_set(): poses built with pnp_ref.make_pose on the cameras of pnp_ref.CAMERAS -- oblique (yaw 60 and 75 degrees), near
fronto-parallel (yaw 0.5 degrees), 0.5 m and 12 m, both plate sizes, the reference camera and the strongly distorted one
(`centred5`, corners of the frame) --, each with its exact projection as float32 pixels, the rotation vector of the
generating pose and an up vector (the camera pitched and rolled) for the yaw block.
"""
import functools
import math

import numpy as np

import pnp_ref as P
from irmv_detection_amd import pose_cov as pc
from irmv_detection_amd import yaw_solve as ys


def camera(cam):
    _, K, D = P.CAMERAS[cam]
    return ys.camera_of(K, D)


def _up(pitch, roll):
    return tuple(float(v) for v in P._rot("z", roll) @ P._rot("x", pitch) @ np.array([0.0, -1.0, 0.0]))


@functools.lru_cache(None)
def hard_set():
    """-> list of dict(name, cam, size, pts float32 [8], R, t, rvec, u)."""
    out = []
    for cam, positions in ((0, ("centre", "tl")), (2, ("centre", "br", "tr"))):
        for size in (0, 1):
            for dist in (0.5, 3.0, 12.0):
                for yaw, pitch, roll in ((60.0, 10.0, 0.0), (-75.0, -20.0, 10.0), (0.5, 0.25, 0.0), (25.0, -15.0, 90.0)):
                    for pname in positions:
                        pos = dict(P.POSITIONS)[pname]
                        R, t = P.make_pose(cam, pos, dist, yaw, pitch, roll)
                        _, K, D = P.CAMERAS[cam]
                        pts = P.project(K, D, R, t, size).reshape(8)
                        if not np.isfinite(pts).all():
                            continue
                        out.append(dict(name=f"{P.CAMERAS[cam][0]}-s{size}-{pname}-d{dist}-y{yaw}-p{pitch}-r{roll}", cam=cam, size=size,
                                        pts=pts, R=R, t=np.asarray(t, np.float64), rvec=P.rvec_of(R), u=_up(15.0 if yaw > 0 else -15.0, 5.0)))
    return out


def reference(case, sigma_px=1.0, with_up=True):
    """pose_cov.pose_cov of a case at its generating pose (the yaw block about the case's up vector)."""
    yaw = (case["rvec"], case["t"], pc.unit(case["u"])) if with_up else None
    return pc.pose_cov(camera(case["cam"]), case["pts"], case["size"], case["rvec"], case["t"], sigma_px, yaw=yaw)


def fields(rec):
    """A record (dict or capi.PoseCov) as (float64 array of its 35 doubles, (state, yaw_state))."""
    d = rec if isinstance(rec, dict) else pc.record_of(rec)
    v = list(d["cov"]) + [d["chi2"], d["sigma_range"]] + list(d["yaw_cov"]) + [d["yaw_chi2"], d["sigma_yaw"]]
    return np.array(v, np.float64), (int(d["state"]), int(d["yaw_state"]))


def same_bits(rec, ref):
    a, sa = fields(rec)
    b, sb = fields(ref)
    return sa == sb and a.tobytes() == b.tobytes()


def first_difference(rec, ref):
    a, sa = fields(rec)
    b, sb = fields(ref)
    bad = [i for i in range(len(a)) if a[i:i + 1].tobytes() != b[i:i + 1].tobytes()]
    return dict(states=(sa, sb), index=bad[:4], dev=[float(a[i]) for i in bad[:4]], ref=[float(b[i]) for i in bad[:4]])


def is_zero_record(rec, state):
    a, s = fields(rec)
    return s == (state, 0) and not a.any() and not np.signbit(a).any()


# ---- the independent checks of the CPU test ---------------------------------------------------------------------------
def residuals(case, w, tau, sigma_px=1.0, up=None):
    """The reference's own eight residuals at the pose perturbed by (w, tau): R <- exp([w]x) R, t <- t + tau.  up: w is a yaw
    angle about it."""
    cam = camera(case["cam"])
    R0 = np.array(pc.rodrigues(case["rvec"])).reshape(3, 3)
    w = np.asarray(w, np.float64) if up is None else float(w) * np.asarray(up, np.float64)
    R = np.array(pc.rodrigues(w)).reshape(3, 3) @ R0
    t = np.asarray(case["t"], np.float64) + np.asarray(tau, np.float64)
    nxy = ys.undistort4(cam, case["pts"])
    _, r = pc.jacobian([float(v) for v in R.reshape(9)], [float(v) for v in t], nxy, case["size"], cam[0], cam[1], sigma_px)
    return np.array(r)


def analytic_jacobian(case, sigma_px=1.0, up=None):
    cam = camera(case["cam"])
    nxy = ys.undistort4(cam, case["pts"])
    J, _ = pc.jacobian(pc.rodrigues(case["rvec"]), [float(v) for v in case["t"]], nxy, case["size"], cam[0], cam[1], sigma_px)
    return np.array(J if up is None else pc.yaw_jacobian(J, up))


def difference_jacobian(case, h, sigma_px=1.0, up=None):
    """Central differences with step h (radians and metres) of residuals()."""
    n = 6 if up is None else 4
    J = np.zeros((8, n))
    for k in range(n):
        p = np.zeros(n); p[k] = h
        wp, tp = (p[:3], p[3:]) if up is None else (p[0], p[1:])
        J[:, k] = (residuals(case, wp, tp, sigma_px, up) - residuals(case, -np.asarray(wp), -tp, sigma_px, up)) / (2.0 * h)
    return J


def rotation_of(ref):
    return np.array(pc.rodrigues(ref)).reshape(3, 3)


def yaw_angle(tau):
    return 2.0 * math.atan(tau)


# ---- the statistical meaning (CPU test) -----------------------------------------------------------------------------------
# Poses that satisfy the yaw model too (tests/pose_prior_set.py's construction): a plate leaning back 15 degrees, the camera
# pitched and rolled; (distance m, yaw deg, pitch deg, roll deg, plate size).  The reference camera.
STAT_CAM = 0
STAT_SIGMA_PX = 0.5
STAT_DRAWS = 2000                       # the sampling error of a variance is sqrt(2 / draws) = 3.2 %
STAT_SAMPLING = math.sqrt(2.0 / STAT_DRAWS)
STAT_POSES = ((2.0, 35.0, 10.0, 0.0, 0), (4.0, -50.0, -15.0, 5.0, 1), (1.2, 20.0, 15.0, -10.0, 0), (3.0, 60.0, 5.0, 0.0, 1),
              (6.0, 40.0, -10.0, 0.0, 1))
N_YAW_POSES = len(STAT_POSES)
# ... and two of pnp_ref.make_pose at the frame's centre (yaw, pitch against the line of sight, roll about it), which no up
# vector describes: the IPPE block alone.  The solver is NOT the maximum-likelihood estimator, and here it shows.
STAT_POSES += ((2.0, 35.0, 10.0, 0.0, 0), (4.0, -50.0, -15.0, 5.0, 1))
STAT_SEPARATION = 10.0                  # the mirror pose is at least this many sigmas of rotation away: the branch is fixed


def stat_pose(k):
    dist, yaw, pitch, roll, size = STAT_POSES[k]
    _, K, D = P.CAMERAS[STAT_CAM]
    if k >= N_YAW_POSES:
        R, t = P.make_pose(STAT_CAM, (640.0, 512.0), dist, yaw, pitch, roll)
        return dict(R=R, t=t, u=None, size=size, pts=P.project(K, D, R, t, size).astype(np.float64))
    Rc = P._rot("z", roll) @ P._rot("x", pitch)
    R = Rc @ P.R_FRONT @ P._rot("z", yaw) @ P._rot("y", 15.0)
    v = np.array([0.1, -0.05, 1.0])
    t = dist * v / np.linalg.norm(v)
    return dict(R=R, t=t, u=pc.unit(Rc @ np.array([0.0, -1.0, 0.0])), size=size, pts=P.project(K, D, R, t, size).astype(np.float64))


def _nearest(sol, R0):
    return int(np.abs(sol["R"][1] - R0).max() < np.abs(sol["R"][0] - R0).max())


def _ml_refine(cam, pts, size, R, t, sigma, steps=3):
    """Gauss-Newton on the model's own residuals from (R, t): the maximum-likelihood pose of the quad."""
    nxy = ys.undistort4(cam, pts)
    for _ in range(steps):
        J, r = pc.jacobian([float(v) for v in R.reshape(9)], [float(v) for v in t], nxy, size, cam[0], cam[1], sigma)
        J, r = np.array(J), np.array(r)
        d = -np.linalg.solve(J.T @ J, J.T @ r)
        R = rotation_of(d[:3]) @ R
        t = t + d[3:]
    return R, t


def sandwich(cam_index, pts, size, R, t, sigma):
    """What the minimiser of the model's residuals scatters by when the noise is drawn in DISTORTED pixels, to first order:
    A^-1 J^T W J A^-1 with W = blockdiag((F G_i^-1)(F G_i^-1)^T), G_i the distortion's own Jacobian d pixel / d normalised at
    corner i (central differences of pnp_ref.distort) and F = diag(fx, fy).  The model sets W = I.  -> the 6 x 6 matrix."""
    _, K, D = P.CAMERAS[cam_index]
    cam = camera(cam_index)
    nxy = np.array(ys.undistort4(cam, pts)).reshape(4, 2)
    J, _ = pc.jacobian([float(v) for v in np.asarray(R).reshape(9)], [float(v) for v in t], [float(v) for v in nxy.reshape(8)], size,
                       cam[0], cam[1], sigma)
    J = np.array(J)
    W = np.zeros((8, 8))
    h = 1e-6
    for i in range(4):
        G = np.array([(P.distort(K, D, nxy[i] + d) - P.distort(K, D, nxy[i] - d)) / (2 * h) for d in (np.array([h, 0.0]), np.array([0.0, h]))]).T
        B = np.diag([cam[0], cam[1]]) @ np.linalg.inv(G)
        W[2 * i:2 * i + 2, 2 * i:2 * i + 2] = B @ B.T
    Ai = np.linalg.inv(J.T @ J)
    return Ai @ J.T @ W @ J @ Ai


@functools.lru_cache(None)
def stat_ippe(k, seed=5):
    """Pose k under STAT_DRAWS draws of corner noise, solved with pnp_ref.solve64 on the branch of the noise-free solution, and
    the same draws refined to the maximum-likelihood pose -> dict(ratio (empirical second moment of (w, tau) about the
    noise-free solution over cov's diagonal, 6), ratio_range, ratio_ml (6), predicted (sandwich()'s diagonal over cov's),
    ratio_sandwich (the refined draws' second moment over sandwich()'s diagonal), separation (mirror distance in sigmas))."""
    p = stat_pose(k)
    _, K, D = P.CAMERAS[STAT_CAM]
    cam = camera(STAT_CAM)
    rng = np.random.default_rng(seed + k)
    q0 = p["pts"].astype(np.float32)
    base = P.solve64(K, D, q0, p["size"])
    g = _nearest(base, p["R"])
    R0, t0 = base["R"][g], base["t"][g]
    ref = pc.pose_cov(cam, q0.reshape(8), p["size"], P.rvec_of(R0), t0, STAT_SIGMA_PX)
    assert ref["state"] == 1
    var = np.diag(pc.full(ref["cov"]))
    sep = float(np.linalg.norm(P.rvec_of(base["R"][1 - g] @ R0.T)) / np.sqrt(var[:3].max()))
    X, M = [], []
    for _ in range(STAT_DRAWS):
        q = (p["pts"] + rng.normal(0, STAT_SIGMA_PX, (4, 2))).astype(np.float32)
        s = P.solve64(K, D, q, p["size"])
        b = _nearest(s, R0)
        X.append(np.concatenate([P.rvec_of(s["R"][b] @ R0.T), s["t"][b] - t0]))
        Rm, tm = _ml_refine(cam, q.reshape(8), p["size"], s["R"][b], s["t"][b], STAT_SIGMA_PX)
        M.append(np.concatenate([P.rvec_of(Rm @ R0.T), tm - t0]))
    X, M = np.array(X), np.array(M)
    d = t0 / np.linalg.norm(t0)
    sw = np.diag(sandwich(STAT_CAM, q0.reshape(8), p["size"], R0, t0, STAT_SIGMA_PX))
    return dict(predicted=sw / var, ratio_sandwich=(M ** 2).mean(0) / sw, ratio=(X ** 2).mean(0) / var, ratio_range=float(((X[:, 3:] @ d) ** 2).mean() / ref["sigma_range"] ** 2),
                ratio_ml=(M ** 2).mean(0) / var, separation=sep)


@functools.lru_cache(None)
def stat_yaw(k, seed=105):
    """Pose k's yaw block against yaw_solve.solve on the same kind of draws -> dict(ratio (psi, tau: 4))."""
    p = stat_pose(k)
    cam = camera(STAT_CAM)
    rng = np.random.default_rng(seed + k)
    s = float(p["R"][:, 0] @ np.array(p["u"]))
    b = ys.solve(cam, p["pts"].astype(np.float32).reshape(8), p["size"], p["u"], s, rounds=6)
    assert b["state"] == 1
    rv = P.rvec_of(b["R"])
    ref = pc.pose_cov(cam, p["pts"].astype(np.float32).reshape(8), p["size"], rv, b["t"], STAT_SIGMA_PX, yaw=(rv, b["t"], p["u"]))
    assert ref["yaw_state"] == 1
    X = []
    for _ in range(STAT_DRAWS):
        q = (p["pts"] + rng.normal(0, STAT_SIGMA_PX, (4, 2))).astype(np.float32)
        y = ys.solve(cam, q.reshape(8), p["size"], p["u"], s, rounds=5)
        assert y["state"] == 1
        X.append([yaw_angle(y["tau"]) - yaw_angle(b["tau"])] + list(y["t"] - b["t"]))
    X = np.array(X)
    return dict(ratio=(X ** 2).mean(0) / np.diag(pc.full(ref["yaw_cov"], 4)), sigma_yaw=ref["sigma_yaw"])
