"""Armor tracks: the arithmetic of k_track.hip, stated once (include/irmv_hip.h, "armor tracks").

Python floats are IEEE doubles and CPython never fuses a multiply into an add, so every expression below is the operation the
kernel performs (built with -ffp-contract=off), in the same order: +, -, *, / and comparisons, nothing else.  Parentheses are
the order; a sum of three terms is written (a + b) + c.

A `Tracker` here is the host reference of one track table: `update()` is one frame and returns what the device delivers -- the
per-detection records, the frame header and the 32-entry snapshot -- and `pack_*` give their bytes.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field

TRACK_CAP = 32
FREE, TENTATIVE, CONFIRMED = 0, 1, 2
# irmv_det_track.state
DET_NONE, DET_MATCHED, DET_STARTED, DET_NO_ROOM = 0, 1, 2, -1
# irmv_track_frame.state
FRAME_OFF, FRAME_OK, FRAME_STALE = 0, 1, -2
# the translation block (rows and columns 3 .. 5) of irmv_pose_cov.cov, the row-major upper triangle of the 6 x 6
POSE_COV_T = ((15, 16, 17), (16, 18, 19), (17, 19, 20))

DET_TRACK_FMT = "<iiIid3d3d"          # irmv_det_track, 72 bytes
FRAME_FMT = "<diiiiiiIi"              # irmv_track_frame, 40 bytes
TRACK_FMT = "<Iiiiiiddd6d36d"         # irmv_track, 384 bytes
DET_TRACK_SIZE, FRAME_SIZE, TRACK_SIZE = 72, 40, 384
assert struct.calcsize(DET_TRACK_FMT) == DET_TRACK_SIZE and struct.calcsize(FRAME_FMT) == FRAME_SIZE and struct.calcsize(TRACK_FMT) == TRACK_SIZE

INF = float("inf")


@dataclass
class Options:
    enable: int = 1
    confirm_hits: int = 3
    max_misses: int = 5
    match_class: int = 1
    gate: float = 16.27          # the 0.999 quantile of chi-square with three degrees of freedom
    max_coast_s: float = 0.5
    accel_sigma: float = 8.0     # m/s^2
    init_vel_sigma: float = 3.0  # m/s
    sigma_lat: float = 0.002
    sigma_rng: float = 0.01


def check_options(o: Options) -> None:
    """What the host refuses (engine_track.cpp check_track_opts): NaN fails every comparison."""
    if o.enable not in (0, 1) or o.match_class not in (0, 1):
        raise ValueError("enable / match_class must be 0 or 1")
    if not (1 <= o.confirm_hits <= 1 << 20) or not (1 <= o.max_misses <= 1 << 20):
        raise ValueError("confirm_hits / max_misses must be in [1, 2^20]")
    for name in ("gate", "max_coast_s", "accel_sigma", "init_vel_sigma", "sigma_lat", "sigma_rng"):
        v = getattr(o, name)
        if not (v > 0.0 and v < INF):
            raise ValueError(f"{name} must be finite and positive")


@dataclass
class Obs:
    """One observation: what the tracker reads of an irmv_det (and of its irmv_pose_cov)."""
    cls: int
    tvec: tuple
    valid: int = 1               # pnp_ok == 1 and armor_valid == 1
    cov: tuple | None = None     # 3 x 3 row-major, camera frame; None: the default noise from sigma_lat / sigma_rng


@dataclass
class Track:
    id: int = 0
    cls: int = 0
    state: int = FREE
    hits: int = 0
    misses: int = 0
    det: int = 0                 # snapshot only: the matched (or starting) detection of this frame, -1: none
    first: float = 0.0
    last_hit: float = 0.0
    stamp: float = 0.0           # the time x and P are valid at
    x: list = field(default_factory=lambda: [0.0] * 6)
    P: list = field(default_factory=lambda: [[0.0] * 6 for _ in range(6)])

    def copy(self) -> "Track":
        return Track(self.id, self.cls, self.state, self.hits, self.misses, self.det, self.first, self.last_hit, self.stamp,
                     list(self.x), [list(r) for r in self.P])


@dataclass
class DetTrack:
    state: int = 0
    track: int = 0
    id: int = 0
    hits: int = 0
    d2: float = 0.0
    pos: tuple = (0.0, 0.0, 0.0)
    vel: tuple = (0.0, 0.0, 0.0)


@dataclass
class Frame:
    stamp: float = 0.0
    state: int = 0
    n_live: int = 0
    n_confirmed: int = 0
    n_started: int = 0
    n_deleted: int = 0
    n_no_room: int = 0
    next_id: int = 1
    reserved: int = 0


def finite(v: float) -> bool:
    return abs(v) < INF          # (a NaN fails too)


def measure(o: Obs, Rw, tw, opt: Options):
    """(eligible, z[3], R[3][3]) of an observation under the camera pose (Rw row-major 3 x 3, tw)."""
    tv = o.tvec
    if o.valid != 1 or not (finite(tv[0]) and finite(tv[1]) and finite(tv[2])) or not (tv[2] > 0.0):
        return False, None, None
    if o.cov is None:
        s1 = opt.sigma_lat * tv[2]
        s2 = opt.sigma_rng * (tv[2] * tv[2])
        C = [[s1 * s1, 0.0, 0.0], [0.0, s1 * s1, 0.0], [0.0, 0.0, s2 * s2]]
    else:
        C = [[o.cov[3 * i + j] for j in range(3)] for i in range(3)]
    z = [((Rw[3 * i] * tv[0] + Rw[3 * i + 1] * tv[1]) + Rw[3 * i + 2] * tv[2]) + tw[i] for i in range(3)]
    M = [[(Rw[3 * i] * C[0][j] + Rw[3 * i + 1] * C[1][j]) + Rw[3 * i + 2] * C[2][j] for j in range(3)] for i in range(3)]
    R = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            R[i][j] = (M[i][0] * Rw[3 * j] + M[i][1] * Rw[3 * j + 1]) + M[i][2] * Rw[3 * j + 2]
            R[j][i] = R[i][j]
    # an observation whose measurement or noise is not usable is not eligible either
    ok = finite(z[0]) and finite(z[1]) and finite(z[2])
    for i in range(3):
        for j in range(i, 3):
            ok = ok and finite(R[i][j])
        ok = ok and R[i][i] > 0.0
    if not ok:
        return False, None, None
    return True, z, R


def predict(x, P, dt: float, accel_sigma: float):
    """x, P (6 x 6, exactly symmetric) moved by dt under constant velocity and white acceleration; returns new lists."""
    q = accel_sigma * accel_sigma
    dt2 = dt * dt
    qpp = (q * (dt2 * dt2)) / 4.0
    qpv = (q * (dt2 * dt)) / 2.0
    qvv = q * dt2
    nx = [x[0] + dt * x[3], x[1] + dt * x[4], x[2] + dt * x[5], x[3], x[4], x[5]]
    N = [[0.0] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            pv = P[i][j + 3] + dt * P[i + 3][j + 3]
            if i == j:
                pv = pv + qpv
            N[i][j + 3] = pv
            N[j + 3][i] = pv
        for j in range(i, 3):
            pp = (P[i][j] + dt * (P[i + 3][j] + P[i][j + 3])) + dt2 * P[i + 3][j + 3]
            vv = P[i + 3][j + 3]
            if i == j:
                pp = pp + qpp
                vv = vv + qvv
            N[i][j] = pp
            N[j][i] = pp
            N[i + 3][j + 3] = vv
            N[j + 3][i + 3] = vv
    return nx, N


def innovation(x, P, z, R):
    """(ok, y[3], Si[3][3]): the residual and the inverse of S = H P H^T + R by cofactors; ok: det S is finite and positive."""
    y = [z[0] - x[0], z[1] - x[1], z[2] - x[2]]
    S = [[P[i][j] + R[i][j] for j in range(3)] for i in range(3)]
    c00 = S[1][1] * S[2][2] - S[1][2] * S[2][1]
    c01 = S[1][2] * S[2][0] - S[1][0] * S[2][2]
    c02 = S[1][0] * S[2][1] - S[1][1] * S[2][0]
    c11 = S[0][0] * S[2][2] - S[0][2] * S[2][0]
    c12 = S[0][1] * S[2][0] - S[0][0] * S[2][1]
    c22 = S[0][0] * S[1][1] - S[0][1] * S[1][0]
    det = (S[0][0] * c00 + S[0][1] * c01) + S[0][2] * c02
    if not (det > 0.0 and det < INF):
        return False, y, None
    i00, i01, i02 = c00 / det, c01 / det, c02 / det
    i11, i12, i22 = c11 / det, c12 / det, c22 / det
    return True, y, [[i00, i01, i02], [i01, i11, i12], [i02, i12, i22]]


def distance2(y, Si) -> float:
    w = [(Si[i][0] * y[0] + Si[i][1] * y[1]) + Si[i][2] * y[2] for i in range(3)]
    return (y[0] * w[0] + y[1] * w[1]) + y[2] * w[2]


def kalman_update(x, P, y, Si):
    """The update with H = [I 0]: K = P H^T Si; x + K y; P - K H P, upper triangle mirrored.  Returns new lists."""
    K = [[(P[i][0] * Si[0][j] + P[i][1] * Si[1][j]) + P[i][2] * Si[2][j] for j in range(3)] for i in range(6)]
    nx = [x[i] + ((K[i][0] * y[0] + K[i][1] * y[1]) + K[i][2] * y[2]) for i in range(6)]
    N = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i, 6):
            N[i][j] = P[i][j] - ((K[i][0] * P[0][j] + K[i][1] * P[1][j]) + K[i][2] * P[2][j])
            N[j][i] = N[i][j]
    return nx, N


def predict_position(tr: Track, t: float, accel_sigma: float):
    """irmv_track_predict: (pos[3], cov[9] row-major) of a live track at stamp t >= tr.stamp."""
    dt = t - tr.stamp
    if tr.state == FREE or not (dt >= 0.0 and dt < INF) or not (accel_sigma > 0.0 and accel_sigma < INF):
        raise ValueError("track is free, t lies before its stamp, or accel_sigma is not positive")
    nx, N = predict(tr.x, tr.P, dt, accel_sigma)
    return nx[:3], [N[i][j] for i in range(3) for j in range(3)]


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class Tracker:
    def __init__(self, opts: Options | None = None):
        self.opt = opts or Options()
        check_options(self.opt)
        self.next_id = 1
        self.reset()

    def reset(self) -> None:
        """The table and its stamp; the id counter goes on."""
        self.tracks = [Track() for _ in range(TRACK_CAP)]
        self.stamped = False
        self.stamp = 0.0

    def snapshot(self, dets_of=None):
        out = []
        for k, tr in enumerate(self.tracks):
            c = tr.copy()
            c.det = -1 if dets_of is None else dets_of[k]
            out.append(c)
        return out

    def update(self, t: float, obs, Rw=IDENTITY, tw=(0.0, 0.0, 0.0)):
        """One frame.  Returns (det_tracks[n], frame, snapshot[32])."""
        opt = self.opt
        n = len(obs)
        dets = [DetTrack() for _ in range(n)]
        if self.stamped and not (t > self.stamp) or not finite(t):
            return dets, Frame(stamp=t, state=FRAME_STALE, next_id=self.next_id), self.snapshot()
        T = self.tracks
        # 1. predict
        if self.stamped:
            dt = t - self.stamp
            for tr in T:
                if tr.state != FREE:
                    tr.x, tr.P = predict(tr.x, tr.P, dt, opt.accel_sigma)
                    tr.stamp = t
        meas = [measure(o, Rw, tw, opt) for o in obs]
        # 2. gated distances
        d2 = {}
        for k, tr in enumerate(T):
            if tr.state == FREE:
                continue
            for i, (ok, z, R) in enumerate(meas):
                if not ok or (opt.match_class != 0 and obs[i].cls != tr.cls):
                    continue
                good, y, Si = innovation(tr.x, tr.P, z, R)
                if not good:
                    continue
                d = distance2(y, Si)
                if d >= 0.0 and d <= opt.gate:
                    d2[(k, i)] = d
        # 3. greedy assignment: the least d2, then the lower track, then the lower observation
        trk_det = [-1] * TRACK_CAP
        obs_trk = [-1] * n
        obs_d2 = [0.0] * n
        while d2:
            k, i = min(d2, key=lambda p: (d2[p], p[0], p[1]))
            trk_det[k], obs_trk[i], obs_d2[i] = i, k, d2[(k, i)]
            d2 = {p: v for p, v in d2.items() if p[0] != k and p[1] != i}
        # 4. update, 5. misses and deletion
        n_deleted = 0
        for k, tr in enumerate(T):
            if tr.state == FREE:
                continue
            i = trk_det[k]
            if i >= 0:
                _, z, R = meas[i]
                _, y, Si = innovation(tr.x, tr.P, z, R)
                tr.x, tr.P = kalman_update(tr.x, tr.P, y, Si)
                tr.hits += 1
                tr.misses = 0
                tr.last_hit = t
                if tr.hits >= opt.confirm_hits:
                    tr.state = CONFIRMED
                dets[i] = DetTrack(DET_MATCHED, k, tr.id, tr.hits, obs_d2[i], tuple(tr.x[:3]), tuple(tr.x[3:]))
            else:
                tr.misses += 1
                if tr.misses > opt.max_misses or (t - tr.last_hit) > opt.max_coast_s:
                    T[k] = Track()
                    n_deleted += 1
        # 6. births, in index order, each in the lowest free entry
        n_started = n_no_room = 0
        for i, (ok, z, R) in enumerate(meas):
            if not ok or obs_trk[i] >= 0:
                continue
            k = next((k for k, tr in enumerate(T) if tr.state == FREE), -1)
            if k < 0:
                dets[i] = DetTrack(DET_NO_ROOM, -1)
                n_no_room += 1
                continue
            v2 = opt.init_vel_sigma * opt.init_vel_sigma
            P = [[0.0] * 6 for _ in range(6)]
            for a in range(3):
                for b in range(3):
                    P[a][b] = R[a][b]
                P[a + 3][a + 3] = v2
            T[k] = Track(self.next_id, obs[i].cls, CONFIRMED if opt.confirm_hits <= 1 else TENTATIVE, 1, 0, 0, t, t, t,
                         [z[0], z[1], z[2], 0.0, 0.0, 0.0], P)
            trk_det[k] = i
            dets[i] = DetTrack(DET_STARTED, k, self.next_id, 1, 0.0, (z[0], z[1], z[2]), (0.0, 0.0, 0.0))
            self.next_id += 1
            n_started += 1
        self.stamped, self.stamp = True, t
        live = sum(tr.state != FREE for tr in T)
        conf = sum(tr.state == CONFIRMED for tr in T)
        frame = Frame(t, FRAME_OK, live, conf, n_started, n_deleted, n_no_room, self.next_id)
        return dets, frame, self.snapshot(trk_det)


def pack_det_track(d: DetTrack) -> bytes:
    return struct.pack(DET_TRACK_FMT, d.state, d.track, d.id, d.hits, d.d2, *d.pos, *d.vel)


def pack_frame(f: Frame) -> bytes:
    return struct.pack(FRAME_FMT, f.stamp, f.state, f.n_live, f.n_confirmed, f.n_started, f.n_deleted, f.n_no_room, f.next_id, f.reserved)


def pack_track(t: Track) -> bytes:
    return struct.pack(TRACK_FMT, t.id, t.cls, t.state, t.hits, t.misses, t.det, t.first, t.last_hit, t.stamp, *t.x, *[v for r in t.P for v in r])
