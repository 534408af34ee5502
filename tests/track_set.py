"""Seeded scenarios for the armor tracker (irmv_detection_amd/tracks.py, k_track.hip).

A scenario is a name, the options and a list of frames (t, R_wc[9], t_wc[3], [tracks.Obs]).  `run_reference` steps a fresh
tracks.Tracker through one and returns, per frame, what the device has to deliver; tests/test_tracks.py asserts the scenario
properties on that, tests/test_gpu_tracks.py compares the kernel's bytes with it.
"""
from __future__ import annotations

import math
import random

from irmv_detection_amd import tracks as T

EYE = T.IDENTITY
ZERO = (0.0, 0.0, 0.0)
DT = 0.01
NAN, INF = float("nan"), float("inf")


def _noisy(rng, p, s_lat=0.002, s_rng=0.01):
    z = p[2]
    return (p[0] + rng.gauss(0.0, s_lat * z), p[1] + rng.gauss(0.0, s_lat * z), p[2] + rng.gauss(0.0, s_rng * z * z))


def _spd(rng, scale):
    a = [[rng.uniform(-1.0, 1.0) for _ in range(3)] for _ in range(3)]
    m = [[sum(a[i][k] * a[j][k] for k in range(3)) * scale + (scale if i == j else 0.0) for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(i):
            m[i][j] = m[j][i]
    return tuple(m[i][j] for i in range(3) for j in range(3))


def moving_targets(seed, n_targets, n_frames, classes=None, with_cov=False):
    rng = random.Random(seed)
    p0 = [(rng.uniform(-1.5, 1.5) + 1.2 * k, rng.uniform(-0.4, 0.4), rng.uniform(2.5, 5.0)) for k in range(n_targets)]
    v0 = [(rng.uniform(-1.0, 1.0), rng.uniform(-0.3, 0.3), rng.uniform(-0.8, 0.8)) for _ in range(n_targets)]
    om = [rng.uniform(1.0, 3.0) for _ in range(n_targets)]
    frames = []
    for f in range(n_frames):
        t = 10.0 + f * DT
        obs = []
        for k in range(n_targets):
            s = math.sin(om[k] * f * DT)
            p = (p0[k][0] + v0[k][0] * f * DT + 0.1 * s, p0[k][1] + v0[k][1] * f * DT, p0[k][2] + v0[k][2] * f * DT)
            cov = _spd(rng, 2e-5) if with_cov and (f + k) % 3 else None
            obs.append(T.Obs(classes[k] if classes else k % 3, _noisy(rng, p), 1, cov))
        frames.append((t, EYE, ZERO, obs))
    return frames


def crossing(match_class):
    """Two targets of classes 1 and 2 on straight lines that cross at frame 40, exact measurements."""
    frames = []
    for f in range(80):
        x = -0.4 + 0.01 * f
        a = T.Obs(1, (x, 0.0, 3.0))
        b = T.Obs(2, (-x, 0.0, 3.0))
        frames.append((1.0 + f * DT, EYE, ZERO, [a, b]))
    return dict(name=f"crossing_mc{match_class}", opts=T.Options(match_class=match_class), frames=frames)


def near_cross(match_class):
    """Two targets of classes 1 and 2, 5 cm apart, that change sides between the first and the second frame: the other class's
    observation is then the nearer one to each track (1 cm against 4 cm, both inside the gate of a one-frame-old track).  With
    the class gate each track keeps its own target; without it the greedy rule takes the nearer pair and the ids swap."""
    xs = [(0.0, 0.05), (0.04, 0.01), (0.05, 0.0), (0.05, 0.0), (0.05, 0.0)]
    frames = [(1.0 + f * DT, EYE, ZERO, [T.Obs(1, (a, 0.0, 3.0)), T.Obs(2, (b, 0.0, 3.0))]) for f, (a, b) in enumerate(xs)]
    return dict(name=f"near_cross_mc{match_class}", opts=T.Options(match_class=match_class), frames=frames)


def coast(max_coast_s=0.5):
    """One static target; the frames come far apart.  Seen at 1.00 .. 1.04; empty frames at 1.24 and 1.44 (two misses, 0.4 s
    since the last hit: kept); seen again at 1.49 (the same id); empty frames at 1.79 (0.3 s: kept) and 2.09 (0.6 s > max_coast_s
    with two misses of the five allowed: deleted); seen at 2.10: a new id."""
    seen = lambda t: (t, EYE, ZERO, [T.Obs(5, (0.3, -0.1, 4.0))])   # noqa: E731
    gone = lambda t: (t, EYE, ZERO, [])                              # noqa: E731
    frames = [seen(1.0 + 0.01 * f) for f in range(5)] + [gone(1.24), gone(1.44), seen(1.49), gone(1.79), gone(2.09), seen(2.10)]
    return dict(name="coast" if max_coast_s == 0.5 else "coast_never", opts=T.Options(max_coast_s=max_coast_s), frames=frames)


def dropout(gap):
    """One target seen for 10 frames, gone for `gap` frames, back for 5."""
    frames = []
    f = 0
    for phase, n in (("on", 10), ("off", gap), ("on", 5)):
        for _ in range(n):
            obs = [T.Obs(3, (0.2 + 0.002 * f, 0.1, 4.0))] if phase == "on" else []
            frames.append((5.0 + f * DT, EYE, ZERO, obs))
            f += 1
    return dict(name=f"dropout_{gap}", opts=T.Options(), frames=frames)


def crowd(n_obs, n_frames=3, seed=5):
    """n_obs eligible observations on a grid 0.5 m apart, classes cycling over 8: more observations than tracks."""
    rng = random.Random(seed)
    frames = []
    for f in range(n_frames):
        obs = [T.Obs(i % 8, _noisy(rng, (-4.0 + 0.5 * (i % 16), -2.0 + 0.5 * (i // 16), 6.0), 0.0005, 0.0002)) for i in range(n_obs)]
        frames.append((2.0 + f * DT, EYE, ZERO, obs))
    return dict(name=f"crowd_{n_obs}", opts=T.Options(), frames=frames)


def free_reuse():
    """Four targets; the second disappears and is deleted, then a fifth appears: entry 1 again, with a fresh id."""
    pts = [(-1.0, 0.0, 3.0), (-0.3, 0.0, 3.0), (0.4, 0.0, 3.0), (1.1, 0.0, 3.0)]
    frames = []
    for f in range(24):
        obs = [T.Obs(0, p) for k, p in enumerate(pts) if not (k == 1 and f >= 4)]
        if f >= 16:
            obs.append(T.Obs(0, (0.0, 0.8, 3.5)))
        frames.append((f * DT + 1.0, EYE, ZERO, obs))
    return dict(name="free_reuse", opts=T.Options(), frames=frames)


def tie():
    """One track at (0, 0, 2); then two observations at exactly equal distance on either side of it."""
    frames = [(1.0, EYE, ZERO, [T.Obs(0, (0.0, 0.0, 2.0))]),
              (1.0 + DT, EYE, ZERO, [T.Obs(0, (0.03125, 0.0, 2.0)), T.Obs(0, (-0.03125, 0.0, 2.0))])]
    return dict(name="tie", opts=T.Options(), frames=frames)


def ineligible():
    bad = [T.Obs(0, (0.0, 0.0, 3.0), 0), T.Obs(0, (NAN, 0.0, 3.0)), T.Obs(0, (0.0, INF, 3.0)), T.Obs(0, (0.0, 0.0, -3.0)),
           T.Obs(0, (0.0, 0.0, 0.0)), T.Obs(0, (0.0, 0.0, 1e200)), T.Obs(0, (0.1, 0.0, 3.0), 1, (NAN,) * 9),
           T.Obs(0, (0.1, 0.0, 3.0), 1, (0.0,) * 9), T.Obs(0, (0.1, 0.0, 3.0), 2)]
    frames = []
    for f in range(6):
        obs = list(bad[: 3 + f]) + [T.Obs(0, (0.0, 0.0, 3.0))] + list(bad[3 + f:])
        frames.append((f * DT + 1.0, EYE, ZERO, obs))
    return dict(name="ineligible", opts=T.Options(), frames=frames)


def stale():
    """Rising stamps with an equal, an earlier and a NaN stamp in the middle."""
    ts = [1.0, 1.01, 1.02, 1.02, 1.005, NAN, 1.03, 1.04]
    frames = [(t, EYE, ZERO, [T.Obs(0, (0.0 + 0.001 * i, 0.0, 3.0)), T.Obs(1, (0.5, 0.0, 3.0))]) for i, t in enumerate(ts)]
    return dict(name="stale", opts=T.Options(), frames=frames)


def static_point(n_frames=300):
    """A static world point seen from a camera that translates and is yawed 0.3 rad: its velocity tends to zero."""
    rng = random.Random(11)
    c, s = math.cos(0.3), math.sin(0.3)
    Rw = (c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c)
    pw = (0.5, -0.2, 5.0)
    frames = []
    for f in range(n_frames):
        tw = (0.6 * f * DT, 0.1 * math.sin(f * DT), -0.3 * f * DT)
        d = (pw[0] - tw[0], pw[1] - tw[1], pw[2] - tw[2])
        pc = (Rw[0] * d[0] + Rw[3] * d[1] + Rw[6] * d[2], Rw[1] * d[0] + Rw[4] * d[1] + Rw[7] * d[2], Rw[2] * d[0] + Rw[5] * d[1] + Rw[8] * d[2])
        frames.append((f * DT + 3.0, Rw, tw, [T.Obs(4, _noisy(rng, pc))]))
    return dict(name="static_point", opts=T.Options(), frames=frames)


def sizes():
    """Frames of 0, 1, 2, 33, 65 and 256 observations (more than tracks, across a wavefront, the cap), every third one invalid."""
    rng = random.Random(17)
    frames = []
    for f, n in enumerate((0, 1, 2, 33, 65, 256, 256, 65, 2, 0)):
        obs = [T.Obs(i % 5, _noisy(rng, (-4.0 + 0.5 * (i % 16), -4.0 + 0.5 * (i // 16), 7.0), 0.0005, 0.0002), 0 if i % 3 == 2 else 1)
               for i in range(n)]
        frames.append((f * DT + 1.0, EYE, ZERO, obs))
    return dict(name="sizes", opts=T.Options(), frames=frames)


def scenarios(long=True):
    out = [dict(name="single_200", opts=T.Options(), frames=moving_targets(1, 1, 200)),
           dict(name="three_200", opts=T.Options(), frames=moving_targets(2, 3, 200)),
           dict(name="three_cov_60", opts=T.Options(confirm_hits=2, max_misses=2, gate=11.34), frames=moving_targets(3, 3, 60, with_cov=True)),
           crossing(1), crossing(0), near_cross(1), near_cross(0), coast(), coast(1e9), dropout(5), dropout(6), crowd(40), free_reuse(), tie(), ineligible(), stale(), static_point(), sizes()]
    if long:
        out.append(dict(name="long_1000", opts=T.Options(), frames=moving_targets(4, 2, 1000, classes=(1, 1))))
    return out


def run_reference(sc):
    """[(det_tracks, frame, snapshot)] per frame, from a fresh reference tracker."""
    tr = T.Tracker(sc["opts"])
    return [tr.update(t, obs, Rw, tw) for t, Rw, tw, obs in sc["frames"]]


def pack_result(res):
    dets, frame, snap = res
    return b"".join(T.pack_det_track(d) for d in dets), T.pack_frame(frame), b"".join(T.pack_track(t) for t in snap)
