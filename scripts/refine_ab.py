"""Refined point source against the keypoint head at 1280 x 1024 -> 640 x 512, in one process (include/irmv_hip.h,
IRMV_POINTS_REFINED).

    python3 scripts/refine_ab.py [out.json]     synthetic frames with 1, 4 and 8 plates whose bars lie at the crafted keypoints;
                                                a KEYPOINT_HEAD engine and a REFINED engine alternated, detect() one frame at a
                                                time: median and p99; the event-timed light_refine launch from irmv_engine_profile;
                                                the cost per frame and per plate

The detections come from a crafted blob (tests/detect_craft.py): the stride-32 level's class bias lights its anchors, boxes are
point-like, the keypoint bias puts one armor-like quad (40 x 24 source pixels) around every anchor.  All 320 anchors of the
level tie in score, so the NMS keeps the first max_det of them in anchor order: a case with n plates runs both engines with
max_det = n and draws the two bars of exactly those n quads -- n detections, n refined.

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FULL, NET = (1280, 1024), (640, 512)
QUAD = ((-20, 12), (-20, -12), (20, -12), (20, 12))     # LB, LT, RT, RB around an anchor's centre, source pixels


def crafted_blob():
    """Stride-32 level lit (20 x 16 = 320 anchors, tied scores: the first max_det in anchor order are kept), the others dark;
    point-like boxes; keypoints QUAD around the anchor's centre: k_net = (2 v + i) 32 = (i + .5) 32 + d / 2."""
    import numpy as np
    import detect_craft as dc
    from irmv_detection_amd import weights
    blob = weights.synthetic_blob(0)
    nc = weights.parse_blob(blob)[0]["nc"]
    lit, dark = dc.dark_bias(nc, float(dc.DARK)), dc.dark_bias(nc, float(dc.DARK))
    lit[4] = 2.0
    kp = ((np.float32(0.5) + np.array(QUAD, np.float32).reshape(8) / np.float32(64.0)) / np.float32(2.0)).astype(np.float32)
    return dc.craft(blob, cls={0: ("bias", dark), 1: ("bias", dark), 2: ("bias", lit)}, box=("bias", dc.POINT_BOXES), kpt=("bias", kp))


def frame_with_plates(n):
    """Bars (4 x 24, top-left pixel cut so that the contour has five points) at the quads of the first n anchors of the level:
    centres (32 + 64 i, 32) in source pixels.  Result coordinates; the buffer is its 180-degree rotation."""
    import numpy as np
    img = np.zeros((FULL[1], FULL[0], 3), np.uint8)
    for i in range(n):
        cx, cy = 32 + 64 * i, 32
        for x0 in (cx - 22, cx + 19):
            img[cy - 12:cy + 12, x0:x0 + 4] = 255
            img[cy - 12, x0] = 0
    return np.ascontiguousarray(img[::-1, ::-1])


def main(args):
    import numpy as np
    from irmv_detection_amd import capi
    from irmv_detection_amd.engine import YoloEngine
    blob = crafted_blob()
    res = {"metric": "refine_ab", "frame": "%dx%d" % FULL, "net": "%dx%d" % NET, "cases": {}}
    for n in (1, 4, 8):
        engs = {k: YoloEngine(None, FULL, weights_blob=blob, net_size=NET[0], net_height=NET[1], point_source=ps, max_det=n)
                for k, ps in (("keypoint", capi.POINTS_KEYPOINT_HEAD), ("refined", capi.POINTS_REFINED))}
        frame = frame_with_plates(n)
        for e in engs.values():
            e.get_src_image_buffer()[:] = frame
            for _ in range(100):
                e.detect()
        flags = [d.reserved for d in engs["refined"].results_raw(0)]
        ms = {k: [] for k in engs}
        for _ in range(12):                       # 12 rounds x 200 frames per engine, engines alternated per round
            for k, e in engs.items():
                for _ in range(200):
                    t0 = time.perf_counter()
                    e.detect()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        case = {"plates": n, "detections": len(flags), "refined": int(sum(f == 1 for f in flags)),
                "detect_ms": {k: dict(frames=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4),
                                      min=round(float(min(v)), 4), sync_launch=engs[k].sync_launch) for k, v in ms.items()}}
        runs = [engs["refined"].profile(0, 1) for _ in range(6)][1:]
        us = [1e3 * st["ms"] for r in runs for st in r if st["name"] == "light_refine"]
        case["light_refine_us_event_timed"] = dict(median=round(float(np.median(us)), 2), min=round(min(us), 2), max=round(max(us), 2), launches=len(us))
        d = case["detect_ms"]
        case["cost_per_frame_us"] = round(1e3 * (d["refined"]["median"] - d["keypoint"]["median"]), 2)
        case["cost_per_plate_us"] = round(case["cost_per_frame_us"] / n, 2)
        res["cases"]["%d_plates" % n] = case
        for e in engs.values():
            e.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
