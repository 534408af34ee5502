"""Measurements of the armor tracks on one GPU, in one visit.

    python3 scripts/tracks_ab.py [--old-lib <parent build of libirmv_hip.so>] [--rounds 4] [--out profiles/tracks_ab.json]

Every leg is a child process (the library is chosen per process through IRMV_LIB_PATH):
  detect    the median of detect() on the 1280 x 1024 benchmark frame on one box: an engine that never enabled the feature, one
            that has it on and one that switched it off again, alternated block by block in one process.  The stamp is set
            outside the timed call.
  flight    three slots in flight (submit slot i mod 3, collect the oldest) with tracking on against off: what the chained
            event costs the overlap, in frames per second.  Both engines set the slot's stamp before every submit.
  kernel    the kernel's time alone: `rocprofv3 --kernel-trace --stats` in a run of its own over irmv_tracker_update calls with
            3, 32 and 256 observations -- the step's kernel, launched without a graph as it is behind a step.
  bench     bench.py's three clocks and the detect() median, feature untouched, a process per library; the order of the two
            libraries alternates from round to round (--old-lib).
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
KERNEL_OBS = (3, 32, 256)
FLIGHT_FRAMES = 600


def _summary(v):
    return dict(median_us=round(statistics.median(v), 2), p10_us=round(sorted(v)[len(v) // 10], 2), p90_us=round(sorted(v)[len(v) * 9 // 10], 2))


def leg_detect():
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    mk = lambda: YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0))   # noqa: E731
    engines = {"never_enabled": mk(), "tracking": mk(), "switched_off": mk()}
    engines["tracking"].set_tracking()
    engines["switched_off"].set_tracking()
    engines["switched_off"].set_tracking(enable=False)
    for e in engines.values():
        e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
        for _ in range(30):
            e.detect()
    t = {k: [] for k in engines}
    stamp = 0.0
    for _ in range(BLOCKS):                       # alternated: a block of each, BLOCKS times
        for k, e in engines.items():
            for _ in range(CALLS):
                stamp += 0.01
                if k == "tracking":
                    e.set_stamp(stamp)
                t0 = time.perf_counter()
                e.detect()
                t[k].append((time.perf_counter() - t0) * 1e6)
    out = {k: dict(_summary(v), detections=len(engines[k].results(0))) for k, v in t.items()}
    frame, _ = engines["tracking"].tracks(0)
    out["tracking_frame"] = dict(state=frame.state, n_live=frame.n_live, n_confirmed=frame.n_confirmed, n_no_room=frame.n_no_room)
    out["cost_us"] = round(out["tracking"]["median_us"] - out["switched_off"]["median_us"], 2)
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def leg_detect_plain():
    """detect() on an engine that never touches the feature: runs under either library."""
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    with YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0)) as e:
        e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
        for _ in range(30):
            e.detect()
        t = []
        for _ in range(BLOCKS * CALLS):
            t0 = time.perf_counter()
            e.detect()
            t.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(_summary(t)))


def leg_flight():
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    out = {}
    engines = {}
    for k in ("off", "on"):
        e = YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0), num_slots=3, num_streams=3)
        if k == "on":
            e.set_tracking()
        for s in range(3):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
        engines[k] = e
    fps = {k: [] for k in engines}
    stamp = 0.0
    for _ in range(4):
        for k, e in engines.items():
            t0 = time.perf_counter()
            for i in range(FLIGHT_FRAMES):
                s = i % 3
                if i >= 3:
                    e.wait_slots(s, 1)
                stamp += 0.01
                e.set_stamp(stamp, s)          # on both engines: the call works before set_tracking, and costs the same wait
                e.submit(s, 1, async_upload=True)
            e.wait()
            fps[k].append(FLIGHT_FRAMES / (time.perf_counter() - t0))
    for k, v in fps.items():
        out[k] = dict(fps=[round(x, 1) for x in v], median_fps=round(statistics.median(v), 1))
    frame, _ = engines["on"].tracks(2)
    out["last_frame_state"] = frame.state
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def leg_kernel():
    """What rocprofv3 traces: 50 irmv_tracker_update calls for each observation count, tracks alive (the observations sit on
    a grid and repeat, so from the second call on every track matches)."""
    from irmv_detection_amd.engine import Tracker
    for n in KERNEL_OBS:
        tr = Tracker()
        obs = [(i % 8, (-4.0 + 0.5 * (i % 16), -4.0 + 0.5 * (i // 16), 7.0), 1, None) for i in range(n)]
        for k in range(50):
            dets, frame, _ = tr.update(1.0 + 0.01 * k, obs)
        print(json.dumps({"observations": n, "matched": sum(d.state == 1 for d in dets), "n_live": frame.n_live, "no_room": frame.n_no_room}), flush=True)
        tr.close()


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
    """-> track_kernel's launches from rocprofv3's kernel trace, in call order: 50 per observation count."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not measured: no rocprofv3"
    d = tempfile.mkdtemp(prefix="tracks_trace_")
    try:
        counted = child([tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--leg", "kernel"], None)
        rows, calls = [], []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(path)) if "track_kernel" in r.get("Name", "")]
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "track_kernel" in r.get("Kernel_Name", ""):
                    calls.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        calls = [us for _, us in sorted(calls)]
        by_n = {}
        for i, n in enumerate(KERNEL_OBS):
            v = calls[50 * i + 1:50 * (i + 1)]        # (the first call of each tracker only starts tracks)
            if v:
                by_n[f"observations_{n}"] = dict(calls=len(v), median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
        return dict(tool="rocprofv3 --kernel-trace --stats, a run of its own (scripts/tracks_ab.py --leg kernel)", counted=counted, stats_rows=rows,
                    track_kernel_by_observations=by_n)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--parts", default="detect,flight,kernel,bench")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = {"detect": leg_detect, "detect_plain": leg_detect_plain, "flight": leg_flight, "kernel": leg_kernel}
    if args.leg:
        return legs[args.leg]()
    from irmv_detection_amd import _build
    out = {"metric": "tracks_ab", "source_hash": _build.source_hash()[:16]}
    parts = args.parts.split(",")
    for name in ("detect", "flight"):
        if name in parts:
            out[name] = child([sys.executable, os.path.abspath(__file__), "--leg", name], None)[-1]
            print(json.dumps(out[name]), flush=True)
    if "kernel" in parts:
        out["kernel_trace"] = kernel_trace()
        print(json.dumps(out["kernel_trace"]), flush=True)
    if "bench" in parts:
        out["bench"] = []
        libs = ([("parent", os.path.abspath(args.old_lib))] if args.old_lib else []) + [("this", None)]
        out["bench_order"] = "round r: " + " then ".join(name for name, _ in libs) + " for even r, reversed for odd r"
        for r in range(args.rounds):
            for name, lib in (libs if r % 2 == 0 else libs[::-1]):
                b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "10", "--no-cpu-baseline"], lib,
                          {"IRMV_BENCH_SKIP": "h2d,config1,config4"})[-1]
                clocks = b.get("fps_by_clock") or {}
                d = child([sys.executable, os.path.abspath(__file__), "--leg", "detect_plain"], lib)[-1]
                row = dict(round=r, lib=name, value=b["value"], three_in_flight=clocks.get("three_in_flight"), one_at_a_time=clocks.get("one_at_a_time"),
                           detect_median_us=d["median_us"])
                out["bench"].append(row)
                print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
