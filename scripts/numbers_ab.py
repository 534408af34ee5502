"""Measurements of the plate numbers on one GPU, in one visit.

    python3 scripts/numbers_ab.py --old-lib <parent build of libirmv_hip.so> [--rounds 3] [--out profiles/numbers_ab.json]

Every leg is a child process (the library is chosen per process through IRMV_LIB_PATH), alternated parent, this, parent,
this ... within the visit:
  post      the post stage alone (run_post: one graph replay, host clock around the synchronous call, median of --reps) on a
            640 x 640 engine with 1, 16 and 100 survivors injected as heads, in four states: never enabled (the parent's
            launches), patches only (the parent's library has this state too), patches plus numbers (one more dependent launch:
            number_step_kernel, model 560 -> 64 -> 9) and both disabled again (the two launches stay and return at once); then
            detect() on the 1280 x 1024 benchmark frame, never enabled, patches only, patches plus numbers.  Run twice: on a
            zero-copy engine (the kernel reads the 592-byte patch records from, and writes the 96-byte records into, pinned host
            memory) and with IRMV_ZERO_COPY_RESULTS=0 (device records and one more D2H copy of max_det records).  The difference
            between the states of one process is the feature's cost; parent against this, never enabled and patches only, is
            the regression check.
  bench     bench.py's three clocks (value, three-in-flight, single-frame), feature untouched.
Without --old-lib only this build runs.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from yaw_solve_ab import SURVIVORS, child, head_with_survivors, timed   # noqa: E402  (the same heads and the same clock)

DIMS = (560, 64, 9)


def model():
    import numpy as np
    from irmv_detection_amd import number_net
    r = np.random.RandomState(30)
    ws = [(r.standard_normal((DIMS[l + 1], DIMS[l])) / np.sqrt(DIMS[l])).astype(np.float32) for l in range(len(DIMS) - 1)]
    bs = [(r.standard_normal(DIMS[l + 1]) * 0.3).astype(np.float32) for l in range(len(DIMS) - 1)]
    return number_net.NumberModel(ws, bs)


def leg_post(reps):
    from irmv_detection_amd import capi, frames, weights
    from irmv_detection_amd.engine import YoloEngine
    has = hasattr(capi.load(), "irmv_engine_set_numbers")
    out = {}
    e = YoloEngine(None, (640, 640), weights_blob=weights.synthetic_blob(0), max_det=256)
    e.get_src_image_buffer()[:] = frames.synthetic_frame(0)[:640, :640]
    e.detect()      # the slot's device frame
    heads = {n: head_with_survivors(e, n) for n in SURVIVORS}
    states = [("never_enabled", None), ("patches_only", "patches")] + ([("patches_numbers", "numbers")] if has else []) + [("disabled", "off")]
    for name, what in states:
        if what == "patches":
            e.set_patches()
        elif what == "numbers":
            e.set_number_model(model())
            e.set_numbers()
        elif what == "off":
            if has:
                e.set_numbers(False)
            e.set_patches(False)
        for n in SURVIVORS:
            e.write_head(heads[n], 0)
            e.run_post(0, 1)
            assert len(e.results(0)) == n
            if what == "numbers":
                out[f"numbers_{n}"] = sum(r.state == 1 for r in e.plate_numbers(0))
            out[f"{name}_{n}"] = timed(lambda: e.run_post(0, 1), reps)
    e.close()
    e = YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0))
    e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
    out["detect_never_enabled"] = timed(lambda: e.detect(), reps)
    e.set_patches()
    out["detect_patches_only"] = timed(lambda: e.detect(), reps)
    if has:
        e.set_number_model(model())
        e.set_numbers()
        out["detect_patches_numbers"] = timed(lambda: e.detect(), reps)
        out["detect_records"] = len(e.results(0))
        out["detect_numbers"] = sum(r.state == 1 for r in e.plate_numbers(0))
    e.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--parts", default="post,post_dev,bench")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg == "post":
        return leg_post(args.reps)
    from irmv_detection_amd import _build
    out = {"metric": "numbers_ab", "source_hash": _build.source_hash()[:16], "model": list(DIMS), "rounds": []}
    libs = ([("parent", os.path.abspath(args.old_lib))] if args.old_lib else []) + [("this", None)]
    parts = args.parts.split(",")
    post = [sys.executable, os.path.abspath(__file__), "--leg", "post", "--reps", str(args.reps)]
    for r in range(args.rounds):
        for name, lib in libs:
            row = dict(round=r, lib=name)
            if "post" in parts:
                row["post_zero_copy"] = child(post, lib)
            if "post_dev" in parts:
                row["post_device_records"] = child(post, lib, {"IRMV_ZERO_COPY_RESULTS": "0"})
            if "bench" in parts:
                b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10", "--no-cpu-baseline"], lib,
                          {"IRMV_BENCH_SKIP": "h2d,config1,config4"})
                clocks = b.get("fps_by_clock") or {}
                row["bench"] = dict(value=b["value"], three_in_flight=clocks.get("three_in_flight"), one_at_a_time=clocks.get("one_at_a_time"))
            out["rounds"].append(row)
            print(json.dumps(row), flush=True)
            if args.out:      # (kept current: a visit that is cut short leaves the rounds it finished)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                open(args.out, "w").write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
