"""The lean-back set of the pose-prior tests (tests/test_pose_prior.py, tests/test_gpu_pose_prior.py) and the crafted head
that injects quads into an engine.  No GPU here.

A plate leaning back 15 degrees on a robot, seen by a camera that is pitched and rolled:

    R = Rc . R_FRONT . rot_z(yaw) . rot_y(+15 deg),   u = Rc . (0, -1, 0)

Rc: pitch +-15 deg about the camera's x axis, roll +-5 deg about its z axis; |yaw| in [10, 60] deg; 1 - 5 m; the plate's
centre inside the 1280 x 1024 frame; Gaussian corner noise of 0.5 px; the reference camera (pnp_ref.CAMERAS[0]); the small
plate.  The outward normal n = column 0 of R then has n . u = -sin 15 deg exactly (NORMAL_UP_ROBOT) whatever Rc and yaw are.
"""
import functools

import numpy as np

import pnp_ref as P
from irmv_detection_amd import pose_prior as pp

CAM, SIZE = 0, 0
S = pp.NORMAL_UP_ROBOT
NOISE = 0.5
N_POSES, SEED = 400, 11
FRAME = (1280, 1024)


def mirror_index(ref, R):
    """Which of the reference's two solutions is the generating pose: the one whose rotation is nearer to R."""
    return int(np.abs(ref["R"][1] - R).max() < np.abs(ref["R"][0] - R).max())


def reference(pts, size=SIZE, cam=CAM):
    """-> (float64 run, mpmath run, classification) of one quad."""
    _, K, D = P.CAMERAS[cam]
    a = P.solve64(K, D, pts, size)
    b = P.solve_mp(K, D, pts, size, hnull=a["hnull"])
    return a, b, P.classify(a, b)


@functools.lru_cache(None)
def lean_back_set(n=N_POSES, seed=SEED):
    """-> list of dict(pts float32 [4, 2], R, t, u, ref (mpmath), cls, gen (index of the generating solution in ref), kept,
    costs (costA, costB of the reference's solutions), pick (the rule on the reference: True = B))."""
    rng = np.random.default_rng(seed)
    _, K, D = P.CAMERAS[CAM]
    out = []
    while len(out) < n:
        pitch, roll = float(rng.choice([-15.0, 15.0])), float(rng.choice([-5.0, 5.0]))
        Rc = P._rot("z", roll) @ P._rot("x", pitch)
        yaw = float(rng.uniform(10, 60) * rng.choice([-1.0, 1.0]))
        dist = float(rng.uniform(1.0, 5.0))
        pos = (float(rng.uniform(0.15, 0.85) * FRAME[0]), float(rng.uniform(0.15, 0.85) * FRAME[1]))
        noise = rng.normal(0, NOISE, (4, 2))
        ray = P._ray(CAM, pos)
        v = np.array([ray[0], ray[1], 1.0]); v /= np.linalg.norm(v)
        R = Rc @ P.R_FRONT @ P._rot("z", yaw) @ P._rot("y", 15.0)
        t = dist * v
        u = Rc @ np.array([0.0, -1.0, 0.0])
        pts = (P.project(K, D, R, t, SIZE).astype(np.float64) + noise).astype(np.float32)
        if pts[:, 0].min() < 0 or pts[:, 0].max() > FRAME[0] or pts[:, 1].min() < 0 or pts[:, 1].max() > FRAME[1]:
            continue
        _, b, c = reference(pts)
        if c["degenerate"]:
            continue
        cA, cB = pp.cost(b["R"][0], u, S), pp.cost(b["R"][1], u, S)
        eA, eB = float(b["err"][0]), float(b["err"][1])
        kept = abs(cA - cB) >= 0.1 and eB < 4 * eA and abs(eB - eA) > 1e-6
        out.append(dict(pts=pts, R=R, t=t, u=u, ref=b, cls=c, gen=mirror_index(b, R), kept=bool(kept), costs=(cA, cB),
                        pick=pp.select(b["R"][0], eA, b["R"][1], eB, u, S, pp.DEFAULT_RATIO, pp.PRIOR)))
    return out


def margin_cases(cases=None):
    """The kept cases whose generating pose is B and on which the reference's rule reports B: min-error reports the mirror
    pose there, the prior the generating one."""
    return [c for c in (cases or lean_back_set()) if c["kept"] and c["gen"] == 1 and c["pick"]]


# ---- the crafted head -------------------------------------------------------------------------------------------------
def cells(net_w, net_h):
    """Stride-8 anchors two cells apart: their 16 px boxes touch and never overlap, so NMS keeps every one."""
    return [(ix, iy) for iy in range(1, net_h // 8, 2) for ix in range(1, net_w // 8, 2)]


def quad_head(e, src, quads, classes=None):
    """A head that makes survivor j report (about) quads[j] with class classes[j] (default j % nc) on a STRETCH engine of
    source size `src`: distinct descending logits, every DFL side in bin 1, keypoint logits v = (k / 8 - (ix, iy)) / 2.
    -> (head, anchors)."""
    nw, nh = e.net_width, e.net_height
    sx, sy = nw / src[0], nh / src[1]
    W8 = nw // 8
    cl = cells(nw, nh)
    assert len(quads) <= len(cl)
    no = e.head_channels
    nc = no - 64 - 8
    head = np.zeros((e.num_anchors, no), np.float32)
    head[:, 64:64 + nc] = -20.0
    head[:, 1:64:16] = 20.0
    anchors = []
    for j, q in enumerate(quads):
        ix, iy = cl[j]
        a = iy * W8 + ix
        head[a, 64 + (j % nc if classes is None else int(classes[j]))] = 8.0 - 0.01 * j
        k = np.asarray(q, np.float64).reshape(4, 2) * [sx, sy]
        head[a, 64 + nc:64 + nc + 8] = ((k / 8 - [ix, iy]) / 2).reshape(8)
        anchors.append(a)
    return head, anchors
