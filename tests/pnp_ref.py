"""An independent planar PnP (IPPE) reference and the pose zoo the PnP tests share.

The solver is restated from the specification, not from the oracle or the device code:
  * undistortion: the contract's fixed-point recipe (x <- (x0 - tangential(x)) / radial(x)), step count a parameter
    (5 is the contract; 50 stands for "converged");
  * Collins & Bartoli 2014: homography of the four correspondences by DLT (null vector of the 8 x 9 system), its
    Jacobian J at the plane origin, R_v (optical axis -> ray through the origin's image) by Rodrigues, gamma = the largest
    singular value of B^-1 J, the last row of the 3 x 2 rotation block from the eigen-decomposition of I - R22^T R22 (both
    signs = the two solutions), translation by least squares, error = rms over the 8 normalised residuals (as cv::IPPE
    states it), model axes from the canonical plane;
  * rotation -> rvec / quaternion by scipy on the SVD-orthonormalised matrix (well conditioned at every angle).

Two precisions: `solve64` (numpy float64: SVD, eigh, lstsq) and `solve_mp` (mpmath, 40 digits: LU null vector, closed
forms, normal equations).  The mpmath run is the truth the bars are measured against; the float64 run is a second fp64
pipeline with another operation order, i.e. a per-pose measure of what fp64 can deliver there.

Terms, stated once:
  AMBIGUOUS        the reference's two solutions have errors within AMBIG_EPS of each other: a solver may return either.
  ILL-CONDITIONED  the float64 reference is more than ILL_EPS (a tenth of the bar) from the mpmath one: the pose's bar is
                   ILL_FACTOR x the float64 reference's own error there.
  DEGENERATE       the 8 x 9 system has lost rank (sigma_8 / sigma_1 < RANK_EPS), the homography itself is singular (two
                   corners coincide, three are collinear: sigma_3 / sigma_1 < RANK_EPS; no plate has such an image) or the
                   reference fails: no pose is defined; only `ok` / finiteness are checked.
"""
import functools

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

from conftest import D_REF, K_REF

BAR = 1e-6            # |d R|, |d tvec| against the reference
AMBIG_EPS = 1e-7      # the rule of test_pnp_batch_random_quads_vs_oracle
ILL_EPS = 1e-7
# Bar of an ill-conditioned pose = ILL_FACTOR x the float64 reference's own error there.  No quad of float32 pixels has been
# found that is ill-conditioned without being DEGENERATE: the zoo's closest-to-singular quads (three corners 2^-11 px off a
# line, two corners 2^-8 px apart) leave the float64 run within 1.7e-10 of the mpmath one, so the factor has no measured ratio.
ILL_FACTOR = 10.0
RANK_EPS = 1e-10
MP_DPS = 40
PIXEL_LIMIT = 2.0 ** 24

HALF_W = (0.135 / 2, 0.225 / 2)      # small, large armor: half width (model y), metres
HALF_H = 0.055 / 2                   # half height (model z)
# canonical plane frame: Xc = y_model, Yc = z_model, Zc = x_model; canonical = P @ model
P_CANON = np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])

# cameras: the reference's; the same K without distortion; one centred on 1280 x 1024 with all five coefficients; and a
# power-of-two camera without distortion, whose normalised coordinates are exact (only the exactly degenerate quads use it)
CAMERAS = (
    ("ref", K_REF, D_REF),
    ("ref_nodist", K_REF, np.zeros(5)),
    ("centred5", np.array([1100.0, 0, 640, 0, 1100, 512, 0, 0, 1]), np.array([-0.2, 0.05, 0.001, -0.0015, -0.01])),
    ("exact", np.array([1024.0, 0, 512, 0, 1024, 512, 0, 0, 1]), np.zeros(5)),
)


def object_points(size):
    """LB, LT, RT, RB in the model frame (x forward, y left, z up)."""
    hy, hz = HALF_W[size], HALF_H
    return np.array([[0, hy, -hz], [0, hy, hz], [0, -hy, hz], [0, -hy, -hz]])


# ------------------------------------------------------------------ camera model
def distort(K, D, xy):
    x, y = xy[..., 0], xy[..., 1]
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    cd = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([K[0] * xd + K[2], K[4] * yd + K[5]], -1)


def project(K, D, R, t, size):
    """R, t (model -> camera) -> the four distorted corner pixels, float32 [4, 2]."""
    pc = object_points(size) @ np.asarray(R).T + np.asarray(t)
    return distort(K, D, pc[:, :2] / pc[:, 2:3]).astype(np.float32)


def undistort(K, D, pts, steps=5):
    """float32 pixels [n, 2] -> normalised coordinates, `steps` fixed-point steps."""
    k1, k2, p1, p2, k3 = D
    x0 = (pts[:, 0].astype(np.float64) - K[2]) / K[0]
    y0 = (pts[:, 1].astype(np.float64) - K[5]) / K[4]
    x, y = x0, y0
    for _ in range(steps):
        r2 = x * x + y * y
        cd = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        x, y = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / cd, (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / cd
    return np.stack([x, y], 1)


def in_range(pts):
    """The input domain: finite float32 pixel coordinates below PIXEL_LIMIT in magnitude.  From 2^24 on a float32 no longer
    resolves a pixel (ulp >= 2 px), so such a quad carries no geometry; fp64 would still make a finite pose of it."""
    with np.errstate(invalid="ignore"):
        return bool((np.abs(np.asarray(pts, np.float32)) < PIXEL_LIMIT).all())


# ------------------------------------------------------------------ float64 solver
def _skew(k):
    return np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])


def _dlt_rows(X, Y, x, y):
    return [[X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x], [0, 0, 0, X, Y, 1, -y * X, -y * Y, -y]]


def solve64(K, D, pts, size, steps=5, sign_rule=True, swap_sizes=False, pick_second=False):
    """-> dict(ok, R [2, 3, 3], t [2, 3], err [2], rank) -- the two solutions, lower error first.  The keyword variants are
    deliberately WRONG solvers (the tests show that the comparison sees them)."""
    pts = np.asarray(pts, np.float32).reshape(4, 2)
    bad = dict(ok=False, R=np.full((2, 3, 3), np.nan), t=np.full((2, 3), np.nan), err=np.full(2, np.nan), rank=0.0, hnull=0)
    if not in_range(pts):
        return bad
    with np.errstate(all="ignore"):
        n = undistort(K, D, pts, steps)
        if not np.isfinite(n).all():
            return bad
        hy, hz = HALF_W[(1 - size) if swap_sizes else size], HALF_H
        cXY = np.array([[hy, -hz], [hy, hz], [-hy, hz], [-hy, -hz]])
        A = np.array([r for (X, Y), (x, y) in zip(cXY, n) for r in _dlt_rows(X, Y, x, y)])
        _, s, vt = np.linalg.svd(A)
        h = vt[-1]
        out = dict(bad, rank=float(s[7] / s[0]) if s[0] > 0 else 0.0, hnull=int(np.argmax(np.abs(h))))
        if not h[8] != 0:
            return out
        H = (h / h[8]).reshape(3, 3)
        sh = np.linalg.svd(H * [hy, hz, 1.0], compute_uv=False)          # (columns scaled to the plate: unit square -> image)
        out["rank"] = min(out["rank"], float(sh[2] / sh[0]))
        p, q = H[0, 2], H[1, 2]
        J = np.array([[H[0, 0] - H[2, 0] * p, H[0, 1] - H[2, 1] * p], [H[1, 0] - H[2, 0] * q, H[1, 1] - H[2, 1] * q]])
        tt = np.hypot(p, q)
        Rv = np.eye(3)
        if tt > 0:
            Kx = _skew(np.array([-q, p, 0.0]) / tt)
            th = np.arctan2(tt, 1.0)
            Rv = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        B = np.array([[1.0, 0, -p], [0, 1, -q]]) @ Rv[:, :2]
        A2 = np.linalg.solve(B, J)
        gam = np.linalg.svd(A2, compute_uv=False)[0]
        R22 = A2 / gam
        M = np.eye(2) - R22.T @ R22
        if sign_rule:
            w, v = np.linalg.eigh(M)
            b = np.sqrt(max(w[1], 0.0)) * v[:, 1]
        else:
            b = np.sqrt(np.maximum(np.diag(M), 0.0))
        Rs, ts, es = [], [], []
        for sg in (1.0, -1.0):
            c0, c1 = np.append(R22[:, 0], sg * b[0]), np.append(R22[:, 1], sg * b[1])
            Rc = Rv @ np.stack([c0, c1, np.cross(c0, c1)], 1)
            rp = cXY @ Rc[:, :2].T                                   # R (X, Y, 0)
            At = np.array([r for x, y in n for r in ([1, 0, -x], [0, 1, -y])])
            bt = np.array([v for (x, y), r in zip(n, rp) for v in (x * r[2] - r[0], y * r[2] - r[1])])
            t = np.linalg.lstsq(At, bt, rcond=None)[0]
            pc = rp + t
            res = pc[:, :2] / pc[:, 2:3] - n
            Rs.append(Rc @ P_CANON); ts.append(t); es.append(np.sqrt((res ** 2).sum() / 8))
        order = [0, 1] if es[0] <= es[1] else [1, 0]
        if pick_second:
            order = order[::-1]
        R, t, e = np.array(Rs)[order], np.array(ts)[order], np.array(es)[order]
        ok = bool(np.isfinite(R[0]).all() and np.isfinite(t[0]).all())
        return dict(out, ok=ok, R=R, t=t, err=e)


# ------------------------------------------------------------------ mpmath solver
def solve_mp(K, D, pts, size, steps=5, hnull=8):
    """The same specification at MP_DPS digits.  `hnull`: which component of the homography's null vector is normalised to
    1 for the LU solve (a pivot hint from the float64 run's SVD; any non-zero component gives the same H)."""
    pts = np.asarray(pts, np.float32).reshape(4, 2)
    bad = dict(ok=False, R=np.full((2, 3, 3), np.nan), t=np.full((2, 3), np.nan), err=np.full(2, np.nan))
    if not in_range(pts):
        return bad
    with mp.workdps(MP_DPS):
        f = mp.mpf
        fx, fy, cx, cy = f(float(K[0])), f(float(K[4])), f(float(K[2])), f(float(K[5]))
        k1, k2, p1, p2, k3 = (f(float(v)) for v in D)
        n = []
        for u, v in pts:
            x0, y0 = (f(float(u)) - cx) / fx, (f(float(v)) - cy) / fy
            x, y = x0, y0
            for _ in range(steps):
                r2 = x * x + y * y
                cd = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
                if cd == 0:
                    return bad
                x, y = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / cd, (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / cd
            n.append((x, y))
        hy, hz = f(HALF_W[size]), f(HALF_H)
        cXY = [(hy, -hz), (hy, hz), (-hy, hz), (-hy, -hz)]
        rows = [r for (X, Y), (x, y) in zip(cXY, n) for r in _dlt_rows(X, Y, x, y)]
        keep = [j for j in range(9) if j != hnull]
        try:
            sol = mp.lu_solve(mp.matrix([[r[j] for j in keep] for r in rows]), mp.matrix([-r[hnull] for r in rows]))
        except (ZeroDivisionError, TypeError):     # singular (mpmath finds no pivot)
            return bad
        h = [f(0)] * 9
        for j, v in zip(keep, sol):
            h[j] = v
        h[hnull] = f(1)
        if h[8] == 0:
            return bad
        H = [v / h[8] for v in h]
        p, q = H[2], H[5]
        J = [[H[0] - H[6] * p, H[1] - H[7] * p], [H[3] - H[6] * q, H[4] - H[7] * q]]
        tt = mp.sqrt(p * p + q * q)
        Rv = mp.eye(3)
        if tt > 0:
            kx, ky = -q / tt, p / tt
            Kx = mp.matrix([[0, 0, ky], [0, 0, -kx], [-ky, kx, 0]])
            th = mp.atan2(tt, 1)
            Rv = mp.eye(3) + mp.sin(th) * Kx + (1 - mp.cos(th)) * Kx * Kx
        B = mp.matrix([[Rv[0, 0] - p * Rv[2, 0], Rv[0, 1] - p * Rv[2, 1]], [Rv[1, 0] - q * Rv[2, 0], Rv[1, 1] - q * Rv[2, 1]]])
        db = B[0, 0] * B[1, 1] - B[0, 1] * B[1, 0]
        if db == 0:
            return bad
        A2 = mp.matrix([[B[1, 1], -B[0, 1]], [-B[1, 0], B[0, 0]]]) * mp.matrix(J) / db
        G = A2.T * A2
        tr, dt = G[0, 0] + G[1, 1], G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
        g2 = (tr + mp.sqrt(max(tr * tr - 4 * dt, f(0)))) / 2
        if not g2 > 0:
            return bad
        R22 = A2 / mp.sqrt(g2)
        M = mp.eye(2) - R22.T * R22
        w, v = mp.eigsy(M)
        iw = 0 if w[0] > w[1] else 1
        sb = mp.sqrt(max(w[iw], f(0)))
        b = (sb * v[0, iw], sb * v[1, iw])
        Rs, ts, es = [], [], []
        for sg in (1, -1):
            c0 = (R22[0, 0], R22[1, 0], sg * b[0])
            c1 = (R22[0, 1], R22[1, 1], sg * b[1])
            c2 = (c0[1] * c1[2] - c0[2] * c1[1], c0[2] * c1[0] - c0[0] * c1[2], c0[0] * c1[1] - c0[1] * c1[0])
            Rc = Rv * mp.matrix([[c0[i], c1[i], c2[i]] for i in range(3)])
            rp = [tuple(Rc[i, 0] * X + Rc[i, 1] * Y for i in range(3)) for X, Y in cXY]
            At = mp.matrix([r for x, y in n for r in ([1, 0, -x], [0, 1, -y])])
            bt = mp.matrix([v_ for (x, y), r in zip(n, rp) for v_ in (x * r[2] - r[0], y * r[2] - r[1])])
            try:
                t = mp.lu_solve(At.T * At, At.T * bt)
            except (ZeroDivisionError, TypeError):     # singular (mpmath finds no pivot)
                return bad
            e = f(0)
            for (x, y), r in zip(n, rp):
                Z = r[2] + t[2]
                if Z == 0:
                    return bad
                e += ((r[0] + t[0]) / Z - x) ** 2 + ((r[1] + t[1]) / Z - y) ** 2
            Rm = np.array([[float(Rc[i, j]) for j in range(3)] for i in range(3)]) @ P_CANON
            Rs.append(Rm); ts.append([float(t[i]) for i in range(3)]); es.append(mp.sqrt(e / 8))
        order = [0, 1] if es[0] <= es[1] else [1, 0]
        R, t = np.array(Rs)[order], np.array(ts)[order]
        e = np.array([float(es[i]) for i in order])
        return dict(ok=bool(np.isfinite(R[0]).all() and np.isfinite(t[0]).all()), R=R, t=t, err=e)


# ------------------------------------------------------------------ rotations
def orthonormal(R):
    u, _, vt = np.linalg.svd(R)
    return u @ np.diag([1, 1, np.linalg.det(u @ vt)]) @ vt


def rvec_of(R):
    return Rotation.from_matrix(orthonormal(R)).as_rotvec()


def quat_of(R):
    return Rotation.from_matrix(orthonormal(R)).as_quat()          # x, y, z, w


def matrix_of(rvec):
    return Rotation.from_rotvec(np.asarray(rvec, np.float64)).as_matrix()


def pi_gap(R):
    """pi - theta of a rotation matrix, well conditioned near pi: theta = 2 atan2(|q_xyz|, |q_w|)."""
    qv = quat_of(R)
    return np.pi - 2 * np.arctan2(np.linalg.norm(qv[:3]), abs(qv[3]))


def quat_branch(R):
    """Which of the four trace / largest-diagonal branches a matrix -> quaternion conversion takes for R."""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "trace"
    return "xyz"[int(np.argmax(np.diag(R)))]


# ------------------------------------------------------------------ the comparison
def pose_error(R, t, refR, reft):
    return max(np.abs(np.asarray(R) - refR).max(), np.abs(np.asarray(t) - reft).max())


def classify(r64, rmp):
    """From the two reference runs alone -> dict(degenerate, ambiguous, ill, err64, bar)."""
    if not rmp["ok"] or not r64["ok"] or r64["rank"] < RANK_EPS:
        return dict(degenerate=True, ambiguous=False, ill=False, err64=np.nan, bar=np.nan)
    ambiguous = bool(abs(rmp["err"][0] - rmp["err"][1]) <= AMBIG_EPS)
    same = max(pose_error(r64["R"][i], r64["t"][i], rmp["R"][i], rmp["t"][i]) for i in (0, 1))
    swap = max(pose_error(r64["R"][i], r64["t"][i], rmp["R"][1 - i], rmp["t"][1 - i]) for i in (0, 1))
    err64 = min(same, swap) if ambiguous else same
    ill = bool(not err64 <= ILL_EPS)
    return dict(degenerate=False, ambiguous=ambiguous, ill=ill, err64=err64, bar=ILL_FACTOR * err64 if ill else BAR)


def check(R, t, ok, rmp, cls):
    """A solver's answer (R matrix, tvec, ok) against the mpmath reference -> (passed, error, which solution).  An
    ambiguous pose may match either solution; every other pose must match the first."""
    if cls["degenerate"]:
        fin = bool(np.isfinite(R).all() and np.isfinite(t).all())
        return (not ok) or fin, 0.0, -1
    if not ok or not (np.isfinite(R).all() and np.isfinite(t).all()):
        return False, np.inf, -1
    e0 = pose_error(R, t, rmp["R"][0], rmp["t"][0])
    if cls["ambiguous"]:
        e1 = pose_error(R, t, rmp["R"][1], rmp["t"][1])
        if e1 < e0:
            return bool(e1 <= cls["bar"]), e1, 1
    return bool(e0 <= cls["bar"]), e0, 0


# ------------------------------------------------------------------ the pose zoo
R_FRONT = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])     # model y (left) -> -x_cam, model z (up) -> -y_cam, normal along +z_cam
POSITIONS = (("pp", None), ("centre", (640.0, 512.0)), ("tl", (60.0, 60.0)), ("tr", (1220.0, 60.0)), ("bl", (60.0, 964.0)),
             ("br", (1220.0, 964.0)), ("partly_out", (-15.0, 300.0)), ("out_neg", (-160.0, -120.0)), ("out_pos", (1400.0, 1100.0)))
PI_LADDER = (0.0, 1e-3, 1e-5, 1e-7, 1e-9, 1e-11)


def _rot(axis, deg):
    return Rotation.from_euler(axis, deg, degrees=True).as_matrix()


@functools.lru_cache(None)
def _ray(cam, pos):
    """Normalised coordinates whose DISTORTED pixel is `pos` (converged fixed point); where the iteration does not settle the
    undistorted nominal ray is used: a position is a label, the generating pose is what the case records."""
    _, K, D = CAMERAS[cam]
    if pos is None:
        return np.zeros(2)
    p = np.array([pos], np.float64)
    a, b = undistort(K, D, p, 200)[0], undistort(K, D, p, 201)[0]
    if np.isfinite(a).all() and np.abs(a - b).max() < 1e-12:
        return a
    return np.array([(pos[0] - K[2]) / K[0], (pos[1] - K[5]) / K[4]])


def _view(xy):
    """Rotation taking the optical axis onto the ray (x, y, 1)."""
    v = np.array([xy[0], xy[1], 1.0]); v /= np.linalg.norm(v)
    k = np.cross([0, 0, 1.0], v)
    s = np.linalg.norm(k)
    if s < 1e-15:
        return np.eye(3), v
    return Rotation.from_rotvec(k / s * np.arctan2(s, v[2])).as_matrix(), v


def make_pose(cam, pos, dist, yaw, pitch, roll):
    """Armor at `dist` metres along the ray through image position `pos`, turned by yaw (about model z), pitch (about model y)
    against the line of sight, and by roll about it: yaw = pitch = 0 is exactly fronto-parallel TO THE RAY, where the two
    IPPE solutions coincide."""
    Rv, v = _view(_ray(cam, pos))
    return Rv @ _rot("z", roll) @ R_FRONT @ _rot("z", yaw) @ _rot("y", pitch), dist * v


# groups built on purpose at (or a hair from) a plate fronto-parallel to its ray: the two solutions coincide BY CONSTRUCTION
FRONTO_GROUPS = ("fronto", "hair", "pi_roll")


def _case(name, group, cam, size, pts, R=None, t=None, noise=0.0):
    return dict(name=name, group=group, cam=cam, size=size, pts=np.asarray(pts, np.float32).reshape(4, 2), R=R, t=t, noise=noise)


def undistortion_converged(case, tol=1e-9):
    """Whether the contract's 5 fixed-point steps have reached the converged (50-step) undistortion at all four points."""
    _, K, D = CAMERAS[case["cam"]]
    with np.errstate(all="ignore"):
        d = np.abs(undistort(K, D, case["pts"], 5) - undistort(K, D, case["pts"], 50)).max()
    return bool(d <= tol)


def _posed(name, group, cam, size, R, t, rng=None, noise=0.0):
    _, K, D = CAMERAS[cam]
    with np.errstate(all="ignore"):
        pts = project(K, D, R, t, size).astype(np.float64)
    if noise:
        pts = pts + rng.normal(0, noise, (4, 2))
    return _case(name, group, cam, size, pts, R, t, noise)


@functools.lru_cache(None)
def zoo(seed=20):
    """The pose zoo: a list of cases, each named by its parameters.  Generated, seeded; nothing is hand-picked but the edges."""
    rng = np.random.default_rng(seed)
    Z = []
    # 1. the bulk: random draws over the whole parameter box
    for i in range(1100):
        cam, size = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        pname, pos = POSITIONS[int(rng.integers(0, len(POSITIONS)))]
        dist = float(np.exp(rng.uniform(np.log(0.3), np.log(12.0))))
        yaw, pitch = float(rng.uniform(-80, 80)), float(rng.uniform(-40, 40))
        roll = float(rng.choice([0.0, 10.0, 90.0, -90.0, 180.0, rng.uniform(-180, 180)]))
        noise = float(rng.choice([0, 0, 0, 0.1, 1.0, 3.0]))
        R, t = make_pose(cam, pos, dist, yaw, pitch, roll)
        Z.append(_posed(f"rand{i}-{CAMERAS[cam][0]}-s{size}-{pname}-d{dist:.2f}-y{yaw:.1f}-p{pitch:.1f}-r{roll:.1f}-n{noise}",
                        "random", cam, size, R, t, rng, noise))
    # 2. the corners of the box
    for cam in range(3):
        for size in (0, 1):
            for dist in (0.3, 12.0):
                for yaw in (-80.0, 80.0):
                    for pitch in (-40.0, 40.0):
                        pname, pos = POSITIONS[(len(Z)) % len(POSITIONS)]
                        R, t = make_pose(cam, pos, dist, yaw, pitch, 0.0)
                        Z.append(_posed(f"edge-{CAMERAS[cam][0]}-s{size}-{pname}-d{dist}-y{yaw}-p{pitch}", "edge", cam, size, R, t))
    # 3. rotation angle pi - eps.  (a) fronto-parallel at the principal point, rolled to 90 deg - sqrt(2) eps (there
    # trace R = -sin roll, so pi - theta = (90 deg - roll) / sqrt 2); (b) R = exp((pi - eps) [n]) for seeded axes n that keep
    # the plate at least 25 deg off edge-on.  The float32 pixels dither the angle the solver sees by ~ 1e-6; the symmetric
    # poses (a) keep it: the tests report the realised pi - theta.
    axes = []
    while len(axes) < 4:
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        if abs(2 * n[2] * n[0]) > 0.45:
            axes.append(n)
    for cam in range(3):
        for size in (0, 1):
            for eps in PI_LADDER:
                for dist in (0.8, 3.0):
                    R = _rot("z", 90.0 - np.degrees(np.sqrt(2.0) * eps)) @ R_FRONT
                    Z.append(_posed(f"pi-roll-{CAMERAS[cam][0]}-s{size}-d{dist}-eps{eps:g}", "pi_roll", cam, size, R, np.array([0, 0, dist])))
                for ai, n in enumerate(axes):
                    R = Rotation.from_rotvec(n * (np.pi - eps)).as_matrix()
                    Z.append(_posed(f"pi-axis{ai}-{CAMERAS[cam][0]}-s{size}-eps{eps:g}", "pi_axis", cam, size, R, np.array([0, 0, 1.5 + ai])))
    # 4. exactly fronto-parallel to the ray (the two solutions coincide), and a hair away
    for cam in range(3):
        for size in (0, 1):
            for pname, pos in POSITIONS[:6]:
                for dist in (0.5, 4.0, 11.0):
                    R, t = make_pose(cam, pos, dist, 0.0, 0.0, 30.0 if dist == 4.0 else 0.0)
                    Z.append(_posed(f"fronto-{CAMERAS[cam][0]}-s{size}-{pname}-d{dist}", "fronto", cam, size, R, t))
                for hair in (1e-6, 1e-3, 0.1):
                    R, t = make_pose(cam, pos, 2.0, hair, -hair / 2, 0.0)
                    Z.append(_posed(f"hair-{CAMERAS[cam][0]}-s{size}-{pname}-yaw{hair:g}", "hair", cam, size, R, t))
    # 5. quads that are no projection of the plate: what a synthetic keypoint head emits
    for cam in (0, 1, 2, 3):
        c = np.array([420.0, 330.0]) if cam < 3 else np.array([512.0, 512.0])
        sq = np.array([[-64.0, 32], [-64, -32], [64, -32], [64, 32]])          # LB, LT, RT, RB (image y down)
        quads = {
            "nonconvex": sq * [[1, 1], [1, 1], [-0.25, 0.25], [1, 1]],
            "crossing": sq[[0, 2, 1, 3]],
            "mirrored": sq[[3, 2, 1, 0]],
            "collinear_h": np.array([[-96.0, 0], [-32, 0], [32, 0], [96, 0]]),
            "collinear_diag": np.array([[-96.0, -96], [-32, -32], [32, 32], [96, 96]]),
            "three_collinear": np.array([[-64.0, 0], [0, 0], [64, 0], [64, 32]]),
            "coincident": np.zeros((4, 2)),
            "two_coincident": np.array([[-64.0, 32], [-64, 32], [64, -32], [64, 32]]),
            # three corners a 2^-k px step off a line: the homography is a hair from singular (not DEGENERATE: ill-conditioned)
            "near_collinear_2^-4": np.array([[-64.0, 0.0625], [0, 0], [64, 0], [64, 32]]),
            "near_collinear_2^-8": np.array([[-64.0, 0.00390625], [0, 0], [64, 0], [64, 32]]),
            "near_collinear_2^-11": np.array([[-64.0, 0.00048828125], [0, 0], [64, 0], [64, 32]]),
            "near_coincident_2^-8": np.array([[-64.0, 32], [-64, 32 - 0.00390625], [64, -32], [64, 32]]),
            "centre_at_infinity": np.array([[0.0, 0], [0, 1024], [-1024, 1024], [1024, 0]]),   # exact camera: g + h = -2
        }
        for size in (0, 1):
            for qn, qd in quads.items():
                Z.append(_case(f"quad-{CAMERAS[cam][0]}-s{size}-{qn}", "quad", cam, size, qd + c))
    return Z


@functools.lru_cache(None)
def zoo_reference(seed=20):
    """-> (r64, rmp, cls) lists over zoo(seed): both reference runs and the classification of every case."""
    r64, rmp, cls = [], [], []
    for c in zoo(seed):
        _, K, D = CAMERAS[c["cam"]]
        a = solve64(K, D, c["pts"], c["size"])
        b = solve_mp(K, D, c["pts"], c["size"], hnull=a["hnull"])
        r64.append(a); rmp.append(b); cls.append(classify(a, b))
    return r64, rmp, cls


def degenerate_flags(K, D, pts, size):
    """Which of the solvers' special branches a quad takes, restated from their definitions: `den` (the unit square -> quad
    map's denominator is zero: RB, RT, LT collinear), `h8` (the plate centre's image at infinity: g + h = -2) and `t0` (the
    plate centre's image is exactly the principal point, p = q = 0: R_v is the identity)."""
    n = undistort(K, D, np.asarray(pts, np.float32).reshape(4, 2))
    lb, lt, rt, rb = n
    d1, d2, s = rb - rt, lt - rt, lb - rb + rt - lt
    den = d1[0] * d2[1] - d1[1] * d2[0]
    if den == 0:
        return {"den"}
    g, h = (s[0] * d2[1] - d2[0] * s[1]) / den, (d1[0] * s[1] - s[0] * d1[1]) / den
    w = 0.5 * g + 0.5 * h + 1.0
    if w == 0:
        return {"h8"}
    centre = (0.5 * (rb - lb + g * rb) + 0.5 * (lt - lb + h * lt) + lb) / w          # image of the unit square's (1/2, 1/2)
    return {"t0"} if centre[0] == 0 and centre[1] == 0 else set()
