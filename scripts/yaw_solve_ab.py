"""Measurements of the constrained pose on one GPU, in one visit.

    python3 scripts/yaw_solve_ab.py --old-lib <parent build of libirmv_hip.so> [--rounds 2] [--out profiles/yaw_solve_ab.json]

Every leg is a child process (the library is chosen per process through IRMV_LIB_PATH), alternated parent, this, parent,
this ... within the visit:
  post      the post stage alone (run_post: one graph replay, host clock around the synchronous call, median of --reps) on a
            640 x 640 engine with 1, 16 and 100 survivors injected as heads, in three states: the feature never enabled (the
            parent's kernels; the only state the parent's library has), enabled (one more dependent launch: yaw_solve_kernel,
            four rounds) and disabled again (the launch stays and returns at once).  The difference between the states of
            one process is the feature's cost; parent against this, never enabled, is the regression check.
  detect    the median of detect() on the 1280 x 1024 benchmark frame, feature never enabled, then enabled.
  bench     bench.py's three clocks (value, three-in-flight, single-frame), feature untouched.
Without --old-lib only this build runs.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SURVIVORS = (1, 16, 100)


def head_with_survivors(e, n):
    """n survivors on the stride-8 level of a 640 x 640 net: anchors four cells apart (16 px boxes, none overlap), an
    armor-like quad around each."""
    import numpy as np
    W8 = e.net_width // 8
    cells = [(ix, iy) for iy in range(2, e.net_height // 8, 4) for ix in range(2, W8, 4)]
    no = e.head_channels
    nc = no - 64 - 8
    head = np.zeros((e.num_anchors, no), np.float32)
    head[:, 64:64 + nc] = -20.0
    head[:, 1:64:16] = 20.0
    quad = np.array([[-3.0, 1.1], [-2.9, -1.0], [3.0, -1.2], [3.1, 1.0]])          # LB, LT, RT, RB in strides, slightly skew
    for j in range(n):
        ix, iy = cells[j]
        head[iy * W8 + ix, 64 + j % nc] = 8.0 - 0.01 * j
        head[iy * W8 + ix, 64 + nc:64 + nc + 8] = (quad / 2).reshape(8)
    return head


def timed(fn, reps, warm=30):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    return dict(median_us=round(statistics.median(t), 2), p10_us=round(t[len(t) // 10], 2), p90_us=round(t[len(t) * 9 // 10], 2))


def leg_post(reps):
    from irmv_detection_amd import capi, frames, weights
    from irmv_detection_amd.engine import YoloEngine
    has = hasattr(capi.load(), "irmv_engine_set_yaw_solve")
    out = {}
    e = YoloEngine(None, (640, 640), weights_blob=weights.synthetic_blob(0), max_det=256)
    heads = {n: head_with_survivors(e, n) for n in SURVIVORS}
    states = [("never_enabled", None)] + ([("enabled", True), ("disabled", False)] if has else [])
    for name, on in states:
        if on is not None:
            e.set_yaw_solve(enable=on)
            e.set_up((0.05, -1.0, 0.1))
        for n in SURVIVORS:
            e.write_head(heads[n], 0)
            e.run_post(0, 1)
            assert len(e.results(0)) == n
            out[f"{name}_{n}"] = timed(lambda: e.run_post(0, 1), reps)
    e.close()
    e = YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0))
    e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
    out["detect_never_enabled"] = timed(lambda: e.detect(), reps)
    if has:
        e.set_yaw_solve()
        out["detect_enabled"] = timed(lambda: e.detect(), reps)
    e.close()
    print(json.dumps(out))


def child(cmd, lib, env_extra=None):
    env = dict(os.environ)
    env.pop("IRMV_LIB_PATH", None)
    if lib:
        env["IRMV_LIB_PATH"] = lib
    env.update(env_extra or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--parts", default="post,bench")
    ap.add_argument("--this-first", action="store_true", help="each round runs this build before the parent's (the order's own effect)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg == "post":
        return leg_post(args.reps)
    from irmv_detection_amd import _build
    out = {"metric": "yaw_solve_ab", "source_hash": _build.source_hash()[:16], "rounds": []}
    libs = ([("parent", os.path.abspath(args.old_lib))] if args.old_lib else []) + [("this", None)]
    if args.this_first:
        libs.reverse()
    parts = args.parts.split(",")
    for r in range(args.rounds):
        for name, lib in libs:
            row = dict(round=r, lib=name)
            if "post" in parts:
                row["post"] = child([sys.executable, os.path.abspath(__file__), "--leg", "post", "--reps", str(args.reps)], lib)
            if "bench" in parts:
                b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10", "--no-cpu-baseline"], lib,
                          {"IRMV_BENCH_SKIP": "h2d,config1,config4"})
                clocks = b.get("fps_by_clock") or {}
                row["bench"] = dict(value=b["value"], three_in_flight=clocks.get("three_in_flight"), one_at_a_time=clocks.get("one_at_a_time"))
            out["rounds"].append(row)
            print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
