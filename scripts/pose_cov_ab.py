"""Measurements of the pose uncertainty on one GPU, in one visit.

    python3 scripts/pose_cov_ab.py [--old-lib <parent build of libirmv_hip.so>] [--rounds 2] [--out profiles/pose_cov_ab.json]

Every leg is a child process (the library is chosen per process through IRMV_LIB_PATH):
  detect    the median of detect() on the 1280 x 1024 benchmark frame on one box: an engine that never enabled the feature
            and one that has it on (and one with the constrained pose beside it), alternated block by block in one process.
  kernel    the kernel's time alone: `rocprofv3 --kernel-trace --stats` in a run of its own over irmv_pnp_pose_cov calls with the
            records of 1 and of 128 frames (32 each), yaw block included: the step kernel's device function on the same grid,
            launched without a graph (leg_kernel says why).
  bench     bench.py's three clocks, feature untouched: parent, this, parent, this ... within the visit (--old-lib).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCKS, CALLS = 6, 100
KERNEL_FRAMES = (1, 128)
RECORDS_PER_FRAME = 32


def _median_us(fn, calls):
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return t


def leg_detect():
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    mk = lambda: YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0))   # noqa: E731
    engines = {"never_enabled": mk(), "pose_cov": mk(), "yaw_solve": mk(), "yaw_solve_and_pose_cov": mk()}
    engines["pose_cov"].set_pose_cov()
    engines["yaw_solve"].set_yaw_solve()
    engines["yaw_solve_and_pose_cov"].set_yaw_solve()
    engines["yaw_solve_and_pose_cov"].set_pose_cov()
    for e in engines.values():
        e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
        for _ in range(30):
            e.detect()
    t = {k: [] for k in engines}
    for _ in range(BLOCKS):                       # alternated: a block of each, BLOCKS times
        for k, e in engines.items():
            t[k] += _median_us(e.detect, CALLS)
    out = {k: dict(median_us=round(statistics.median(v), 2), p10_us=round(sorted(v)[len(v) // 10], 2), p90_us=round(sorted(v)[len(v) * 9 // 10], 2),
                   detections=len(engines[k].results(0))) for k, v in t.items()}
    out["records_with_state_1"] = sum(c.state == 1 for c in engines["yaw_solve_and_pose_cov"].pose_covs(0))
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def leg_kernel():
    """What rocprofv3 traces: 50 calls of irmv_pnp_pose_cov for each size -- 32 records a frame, the yaw block included.  The
    stand-alone kernel runs the step kernel's device function (posecov_wave) on the same grid of one wave per record; it is
    traced in place of the step because a step is a hipGraphLaunch, and the profiler's packet walk over graph launches is
    what DESIGN.md section 9 found faulting on the host (the committed profiles keep graph replays of single steps out of
    traced runs)."""
    import numpy as np
    import pnp_ref as P
    import pose_prior_set as L
    from irmv_detection_amd.engine import PnPSolver
    cases = L.lean_back_set(64)[:RECORDS_PER_FRAME]
    _, K, D = P.CAMERAS[L.CAM]
    s = PnPSolver(K, list(D))
    for n in KERNEL_FRAMES:
        pick = [cases[i % len(cases)] for i in range(n * RECORDS_PER_FRAME)]
        pts = np.array([c["pts"].reshape(8) for c in pick], np.float32)
        rv = np.array([P.rvec_of(c["R"]) for c in cases])[[i % len(cases) for i in range(len(pick))]]
        tv = np.array([c["t"] for c in pick])
        for _ in range(50):
            out = s.pose_cov(pts, rv, tv, L.SIZE, up=cases[0]["u"])
        print(json.dumps({f"records_state_1_of_{n}_frames": sum(c.state == 1 for c in out), f"yaw_state_1_of_{n}_frames": sum(c.yaw_state == 1 for c in out),
                          "records": len(out)}), flush=True)
    s.close()


def child(cmd, lib, env_extra=None, want_json=True):
    env = dict(os.environ)
    env.pop("IRMV_LIB_PATH", None)
    if lib:
        env["IRMV_LIB_PATH"] = lib
    env.update(env_extra or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or (want_json and not lines):
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return [json.loads(l) for l in lines]


def kernel_trace():
    """-> the rows of rocprofv3's kernel stats that name the feature's kernels, and what the traced process counted."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not measured: no rocprofv3"
    d = tempfile.mkdtemp(prefix="pose_cov_trace_")
    try:
        counted = child([tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--leg", "kernel"], None)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(path)) if "pose_cov" in r.get("Name", "") or "yaw_solve" in r.get("Name", "")]
        calls = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "pose_cov" in r.get("Kernel_Name", ""):
                    key = "grid_%s_x_%s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Grid_Size_Y", "?"))
                    calls.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        per_grid = {k: dict(calls=len(v), median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in calls.items()}
        return dict(tool="rocprofv3 --kernel-trace --stats, a run of its own (scripts/pose_cov_ab.py --leg kernel)", frames=list(KERNEL_FRAMES),
                    records_per_frame=RECORDS_PER_FRAME, counted=counted, stats_rows=rows, pose_cov_points_kernel_by_grid=per_grid)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--parts", default="detect,kernel,bench")
    ap.add_argument("--this-first", action="store_true", help="each round runs this build before the parent's (the order's own effect)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg == "detect":
        return leg_detect()
    if args.leg == "kernel":
        return leg_kernel()
    from irmv_detection_amd import _build
    out = {"metric": "pose_cov_ab", "source_hash": _build.source_hash()[:16]}
    parts = args.parts.split(",")
    if "detect" in parts:
        out["detect"] = child([sys.executable, os.path.abspath(__file__), "--leg", "detect"], None)[-1]
        print(json.dumps(out["detect"]), flush=True)
    if "kernel" in parts:
        out["kernel_trace"] = kernel_trace()
        print(json.dumps(out["kernel_trace"]), flush=True)
    if "bench" in parts:
        out["bench"] = []
        libs = ([("parent", os.path.abspath(args.old_lib))] if args.old_lib else []) + [("this", None)]
        if args.this_first:
            libs.reverse()
        out["bench_order"] = [name for name, _ in libs]
        for r in range(args.rounds):
            for name, lib in libs:
                b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10", "--no-cpu-baseline"], lib,
                          {"IRMV_BENCH_SKIP": "h2d,config1,config4"})[-1]
                clocks = b.get("fps_by_clock") or {}
                row = dict(round=r, lib=name, value=b["value"], three_in_flight=clocks.get("three_in_flight"), one_at_a_time=clocks.get("one_at_a_time"))
                out["bench"].append(row)
                print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
