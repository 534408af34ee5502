"""A/B of the network input shape on one GPU: 640 x 640 against 640 x 512 for the 1280 x 1024 camera.

    python3 scripts/rect_ab.py [--steps 60] [--repeats 5] [--single 300]

Throughput: bench.py's batched step shape -- 256 seeded synthetic frames per step resident in HBM, the engine's default
streams (two), engines tuned at creation -- both shapes in the same process, timed in alternation, `repeats` rounds of
`steps` steps each.  Latency: detect() on single-slot engines of both shapes, alternating likewise.  Prints one JSON line:
the median FPS of each shape and each mode, the spread (min, max) across rounds, and the event-timed kernel ms
(irmv_engine_profile) of one stream's sub-batch, per kernel family, and of one single-frame step: a speed-up below the 20 %
cut in conv FLOPs can be read from them.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irmv_detection_amd import frames, weights  # noqa: E402
from irmv_detection_amd.engine import YoloEngine  # noqa: E402

SHAPES = {"640x640": (640, 640), "640x512": (640, 512)}


def family(name):
    """kernel name -> family (tile shapes and fused-epilogue suffixes dropped)"""
    return re.sub(r"(_mt\d.*|_nt\d.*|_x\d+|\+1x1)$", "", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single", type=int, default=300, help="detect() calls per round and shape")
    args = ap.parse_args()
    blob = weights.synthetic_blob(0)
    B = args.frames
    out = {"metric": "rect_ab", "src": "1280x1024", "frames_per_step": B, "steps": args.steps, "repeats": args.repeats}

    # ---- batched throughput ----
    engs = {k: YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=B, net_size=w, net_height=h) for k, (w, h) in SHAPES.items()}
    for e in engs.values():
        for s in range(B):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
        e.submit(0, B, h2d=True)
        e.wait()
        for _ in range(args.warmup):
            e.submit(0, B, h2d=False)
        e.wait()
    fps = {k: [] for k in SHAPES}
    for _ in range(args.repeats):
        for k, e in engs.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.submit(0, B, h2d=False)
            e.wait()
            fps[k].append(B * args.steps / (time.perf_counter() - t0))
    prof = {}
    for k, e in engs.items():
        share = -(-B // e.num_streams)
        runs = [e.profile(0, share) for _ in range(4)][1:]
        agg = {}
        for run in runs:
            for st in run:
                f = family(st["name"])
                agg[f] = agg.get(f, 0.0) + st["ms"] / len(runs)
        prof[k] = dict(frames=share, launches=len(runs[0]), total_ms=round(sum(agg.values()), 3),
                       by_family_ms={f: round(v, 3) for f, v in sorted(agg.items(), key=lambda kv: -kv[1])})
        out.setdefault("anchors", {})[k] = e.num_anchors
        out.setdefault("streams", {})[k] = e.num_streams
    for e in engs.values():
        e.close()

    # ---- single-frame detect() ----
    ones = {k: YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=1, net_size=w, net_height=h) for k, (w, h) in SHAPES.items()}
    for e in ones.values():
        e.get_src_image_buffer(0)[:] = frames.synthetic_frame(0)
        for _ in range(50):
            e.detect()
    single = {k: [] for k in SHAPES}
    for _ in range(args.repeats):
        for k, e in ones.items():
            t0 = time.perf_counter()
            for _ in range(args.single):
                e.detect()
            single[k].append(args.single / (time.perf_counter() - t0))
    prof_one = {}
    for k, e in ones.items():
        runs = [e.profile(0, 1) for _ in range(4)][1:]
        prof_one[k] = dict(launches=len(runs[0]), kernel_ms=round(sum(st["ms"] for r in runs for st in r) / len(runs), 4),
                           detect_ms=round(1e3 / statistics.median(single[k]), 4))
    for e in ones.values():
        e.close()

    def summary(v):
        return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
    out["batched_fps"] = {k: summary(v) for k, v in fps.items()}
    out["single_frame_fps"] = {k: summary(v) for k, v in single.items()}
    out["speedup_batched"] = round(statistics.median(fps["640x512"]) / statistics.median(fps["640x640"]), 4)
    out["speedup_single"] = round(statistics.median(single["640x512"]) / statistics.median(single["640x640"]), 4)
    out["profile_one_sub_batch"] = prof
    out["profile_single_frame"] = prof_one   # event-timed kernel sum of one eager step vs the detect() wall clock
    print(json.dumps(out))


if __name__ == "__main__":
    main()
