"""Measurements of the class policy on one GPU, in one visit.

    python3 scripts/class_policy_ab.py --old-lib <parent build of libirmv_hip.so> [--rounds 3] [--out profiles/class_policy_ab.json]

  regress   this build against the parent commit's library, alternated old, new, old, new ... within the visit, each run a
            child process (the library is chosen per process through IRMV_LIB_PATH): bench.py's `value` (batched, frames
            resident in HBM), and on a three-slot engine shaped like the reference node's the three-in-flight clock and the
            single-frame clock (frame resident).  Reported per library with min / median / max: the spread of the parent's
            own runs is what a difference has to be read against.
  mask      what a colour mask buys: the bench frames on a blob whose class finals are shifted by --shift (so that candidates
            exist), policy -1 (both colours) against enemy 0, alternated on ONE engine: candidate counts per frame (the
            engine's n_candidates -- tests/test_gpu_class_policy.py holds it to the CPU oracle's; no (tile, image) share is
            computed), the batched frames/s, and the event-timed launches behind the class carriers plus nms_pnp
            (irmv_engine_profile).
  change    median and p99 of irmv_engine_set_class_policy on an idle engine, against irmv_engine_set_window on the same box.
Without --old-lib the regress part is left out; --parts regress runs that part alone (a further visit, written to a file
of its own: profiles/class_policy_ab_regress.json).  Child legs: --leg clocks.
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


def summary(v, nd=1):
    return dict(min=round(min(v), nd), median=round(statistics.median(v), nd), max=round(max(v), nd), runs=[round(x, nd) for x in v])


def leg_clocks():
    """Child: the two latency-side clocks of bench.py's three-slot engine, on whichever library IRMV_LIB_PATH names."""
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    e = YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0), num_slots=3)
    for s in range(3):
        e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
    for _ in range(30):
        e.detect(0)
    t = time.perf_counter()
    for _ in range(300):
        e.submit(0, 1, h2d=False); e.wait()
    single_ms = (time.perf_counter() - t) / 300 * 1e3
    for j in range(2):
        e.submit(j, 1, async_upload=True)
    n = 900
    t = time.perf_counter()
    for i in range(n):
        e.submit((i + 2) % 3, 1, async_upload=True)
        e.wait_slots(i % 3, 1)
    e.wait()
    three = n / (time.perf_counter() - t)
    e.close()
    print(json.dumps(dict(single_frame_resident_ms=single_ms, three_in_flight_fps=three)))


def child(cmd, lib):
    env = dict(os.environ)
    env.pop("IRMV_LIB_PATH", None)
    if lib:
        env["IRMV_LIB_PATH"] = lib
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1])


def regress(old_lib, rounds, steps):
    got = {k: dict(value=[], three=[], single=[]) for k in ("old", "new")}
    os.environ["IRMV_BENCH_SKIP"] = "h2d,latency,config1,config4"      # (the children inherit it: bench.py's batched leg alone)
    for _ in range(rounds):
        for k, lib in (("old", old_lib), ("new", None)):
            b = child([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "10", "--no-cpu-baseline"], lib)
            c = child([sys.executable, os.path.abspath(__file__), "--leg", "clocks"], lib)
            got[k]["value"].append(b["value"])
            got[k]["three"].append(c["three_in_flight_fps"])
            got[k]["single"].append(c["single_frame_resident_ms"])
    out = {}
    for name, key, nd in (("bench_value_fps", "value", 1), ("three_in_flight_fps", "three", 1), ("single_frame_resident_ms", "single", 4)):
        o, n = got["old"][key], got["new"][key]
        out[name] = dict(parent=summary(o, nd), this=summary(n, nd), parent_spread_pct=round(100 * (max(o) - min(o)) / statistics.median(o), 2),
                         this_spread_pct=round(100 * (max(n) - min(n)) / statistics.median(n), 2),
                         median_change_pct=round(100 * (statistics.median(n) / statistics.median(o) - 1), 2))
    return out


def behind_the_carriers(st):
    """The launches whose work follows the candidates: the Detect box and keypoint branches, the scan and nms_pnp."""
    return (st["layer"].startswith("model.22.") and (".cv2." in st["layer"] or ".cv4." in st["layer"])) or st["name"].startswith(("kpt3", "nms", "scan"))


def mask(shift, B, steps, repeats):
    import numpy as np
    import detect_craft as dc
    from irmv_detection_amd import class_policy as cp, frames, weights
    from irmv_detection_amd.engine import YoloEngine
    blob = dc.craft(weights.synthetic_blob(0), cls=("shift", shift))
    e = YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=B)
    for s in range(B):
        e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
    e.submit(0, B, h2d=True)
    e.wait()
    pols = {"both (-1)": cp.enemy(-1, 0.25), "enemy 0": cp.enemy(0, 0.25)}
    res = {k: dict(fps=[]) for k in pols}
    share = -(-B // e.num_streams)
    for r in range(repeats):
        for k, p in pols.items():
            e.set_class_policy(p)
            for _ in range(5):
                e.submit(0, B, h2d=False)
            e.wait()
            t = time.perf_counter()
            for _ in range(steps):
                e.submit(0, B, h2d=False)
            e.wait()
            res[k]["fps"].append(B * steps / (time.perf_counter() - t))
            if r == 0:
                n = [e.read_raw(s)["n_candidates"] for s in range(B)]
                dets = [e.read_raw(s)["num_dets"] for s in range(B)]
                res[k]["candidates_per_frame"] = dict(min=int(min(n)), median=float(statistics.median(n)), max=int(max(n)), total=int(sum(n)))
                res[k]["detections_per_frame_median"] = float(statistics.median(dets))
                runs = [e.profile(0, share) for _ in range(4)][1:]
                rows = {}
                for run in runs:
                    for st in run:
                        if behind_the_carriers(st):
                            key = f"{st['layer']} [{st['name']}]"
                            rows[key] = rows.get(key, 0.0) + st["ms"] / len(runs)
                res[k]["launch_ms_one_share"] = {a: round(b, 4) for a, b in rows.items()}
                res[k]["launch_ms_one_share_sum"] = round(sum(rows.values()), 4)
                res[k]["step_ms_one_share_all_launches"] = round(sum(st["ms"] for run in runs for st in run) / len(runs), 4)
    for k in pols:
        res[k]["fps"] = summary(res[k]["fps"])
    e.close()
    return dict(shift=shift, frames_per_step=B, frames_in_share=share, steps=steps, repeats=repeats, policies=res,
                note="synthetic weights shifted so that candidates exist: their class mix is not a match's")


def change(n):
    import numpy as np
    from irmv_detection_amd import class_policy as cp, frames, weights
    from irmv_detection_amd.engine import YoloEngine
    e = YoloEngine(None, (1280, 1024), weights_blob=weights.synthetic_blob(0), num_slots=3, window=(640, 512))
    e.get_src_image_buffer(0)[:] = frames.synthetic_frame(0)
    e.detect(0)
    pols = [cp.enemy(0, 0.25), cp.enemy(1, 0.25)]
    out = {}
    for name, fn in (("set_class_policy", lambda i: e.set_class_policy(pols[i & 1])), ("set_window", lambda i: e.set_window(100 + (i & 63), 80 + (i & 31), 0))):
        for i in range(50):
            fn(i)
        t = []
        for i in range(n):
            t0 = time.perf_counter()
            fn(i)
            t.append((time.perf_counter() - t0) * 1e6)
        out[name + "_us"] = dict(median=round(float(np.median(t)), 2), p99=round(float(np.percentile(t, 99)), 2), calls=n,
                                 note="through the Python mirror (ctypes), idle engine")
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--shift", type=float, default=1.75)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="regress,mask,change")
    args = ap.parse_args()
    if args.leg == "clocks":
        return leg_clocks()
    from irmv_detection_amd import _build
    out = {"metric": "class_policy_ab", "source_hash": _build.source_hash()[:16]}
    parts = args.parts.split(",")
    if "change" in parts:
        out["change"] = change(2000)
    if "mask" in parts:
        out["mask"] = mask(args.shift, args.frames, args.steps, args.rounds)
    if "regress" in parts and args.old_lib:
        out["regress"] = regress(os.path.abspath(args.old_lib), args.rounds, args.steps)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
