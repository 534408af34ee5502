"""Frame metering at 1280 x 1024 (csrc/k_meter.hip): what the op costs, and what it costs an engine that never asks.

    python3 scripts/metering_ab.py kernel <order.json>   the program of a `rocprofv3 --kernel-trace` run of its own: per case
                                                         CALLS on-demand meter() calls of one frame, in the order written to
                                                         order.json.  Cases: HWC VIEW and Bayer RAW x steps 1, 2, 4 x four
                                                         frames (random, tests/golden/rm_test.jpg, all 0, all 255) x the two
                                                         forms of the LDS add (IRMV_METER_MERGE=0 / 1)
    python3 scripts/metering_ab.py batch [out.json]      the same cases on 128 frames in one step: the frame_meter row of
                                                         irmv_engine_profile (an event pair around four launches)
    python3 scripts/metering_ab.py time [out.json]       detect() one frame at a time, and three async single-slot submits in
                                                         flight: an engine with metering enabled against one without, the two
                                                         alternated; median and p99
    python3 scripts/metering_ab.py merge <order.json> <kernel_trace.csv | -> <batch.json | -> <time.json | -> <ab_lib lines | -> [out.json]
                                                         the frame_meter dispatches of that trace, case by case, stated as bytes
                                                         over time against the 6.29 TB/s copy line, the uniform frames as a ratio
                                                         to the random one; the other files as they are ("-": not measured)

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = (1280, 1024)
CALLS = 10
STEPS = (1, 2, 4)
FRAMES = ("random", "rm_test", "zeros", "ones255")
COPY_LINE_TBS = 6.29
ALTERNATIONS, DETECTS = 6, 60


def _frame(name, raw):
    import numpy as np
    h, w = SIZE[1], SIZE[0]
    if name == "random":
        f = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif name == "rm_test":
        from PIL import Image
        f = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "rm_test.jpg")).convert("RGB").resize((w, h)))
    else:
        f = np.full((h, w, 3), 0 if name == "zeros" else 255, np.uint8)
    if raw:
        from irmv_detection_amd import bayer
        return bayer.mosaic(f, "RGGB")
    return f


def _engine(raw, merge=None, slots=1):
    from irmv_detection_amd import weights
    from irmv_detection_amd.engine import YoloEngine
    if merge is None:
        os.environ.pop("IRMV_METER_MERGE", None)
    else:
        os.environ["IRMV_METER_MERGE"] = "1" if merge else "0"
    e = YoloEngine(None, SIZE, weights_blob=weights.synthetic_blob(0), num_slots=slots, src_format="RGGB" if raw else 0)
    os.environ.pop("IRMV_METER_MERGE", None)
    return e


def _bytes_read(raw, step):
    """The bytes the sampled rows hold: every step-th row of the view (VIEW), every step-th pair of rows (RAW)."""
    rows = -(-SIZE[1] // step) if not raw else 2 * -(-(SIZE[1] // 2) // step)
    return rows * SIZE[0] * (1 if raw else 3)


def cmd_kernel(args):
    order = []
    for raw in (False, True):
        for merge in (False, True):
            e = _engine(raw, merge)
            for name in FRAMES:
                e.get_src_image_buffer()[:] = _frame(name, raw)
                for step in STEPS:
                    for _ in range(CALLS):
                        e.meter("raw" if raw else "view", None, step)
                    order.append(dict(domain="raw" if raw else "view", merge=int(merge), frame=name, step=step, calls=CALLS, frames=1,
                                      bytes_read=_bytes_read(raw, step)))
            e.close()
    open(args[0], "w").write(json.dumps(order) + "\n")


def cmd_batch(args):
    import numpy as np
    n, res = 128, []
    for raw in (False, True):
        for merge in (False, True):
            e = _engine(raw, merge, slots=n)
            for name in ("random", "zeros", "ones255"):
                f = _frame(name, raw)
                for s in range(n):
                    e.get_src_image_buffer(s)[:] = f
                e.submit(0, n)
                e.wait()
                for step in STEPS:
                    e.set_metering("raw" if raw else "view", None, step)
                    ms = [[r["ms"] for r in e.profile(0, n) if r["name"] == "frame_meter"][0] for _ in range(5)]
                    med = float(np.median(ms))
                    res.append(dict(domain="raw" if raw else "view", merge=int(merge), frame=name, step=step, frames=n, ms_median=round(med, 5),
                                    ms_all=[round(v, 5) for v in ms], tb_per_s=round(n * _bytes_read(raw, step) / (med * 1e-3) / 1e12, 4)))
            e.close()
    txt = json.dumps(dict(metric="frame_meter, 128 frames in one step, irmv_engine_profile", rows=res), indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def _stats(v):
    import numpy as np
    return dict(calls=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4), min=round(float(min(v)), 4))


def cmd_time(args):
    import numpy as np
    from irmv_detection_amd import frames
    res = {"metric": "metering_ab time", "frame": "%dx%d" % SIZE, "alternations": ALTERNATIONS}
    pair = [_engine(False, None, 3), _engine(False, None, 3)]     # [0] never asks, [1] meters the whole view at step 1
    for e in pair:
        for s in range(3):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
    pair[1].set_metering("view", None, 1)
    for e in pair:
        for _ in range(30):
            e.detect(0)
    det = ([], [])
    rounds = ([], [])
    for _ in range(ALTERNATIONS):
        for i, e in enumerate(pair):
            v = []
            for _ in range(DETECTS):
                t0 = time.perf_counter()
                e.detect(0)
                v.append((time.perf_counter() - t0) * 1e3)
            det[i].extend(v)
            rounds[i].append(float(np.median(v)))
    res["detect_one_frame_ms"] = dict(not_enabled=_stats(det[0]), enabled=_stats(det[1]), not_enabled_round_medians=[round(v, 4) for v in rounds[0]],
                                      enabled_round_medians=[round(v, 4) for v in rounds[1]])
    asy = ([], [])
    for _ in range(ALTERNATIONS):
        for i, e in enumerate(pair):
            for _ in range(DETECTS // 3):
                t0 = time.perf_counter()
                for s in range(3):
                    e.submit(s, 1, async_upload=True)
                for s in range(3):
                    e.wait_slots(s, 1)
                asy[i].append((time.perf_counter() - t0) * 1e3)
    res["three_async_single_slot_submits_ms"] = dict(not_enabled=_stats(asy[0]), enabled=_stats(asy[1]))
    for e in pair:
        e.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def cmd_merge(args):
    import numpy as np
    order = json.load(open(args[0]))
    res = {"metric": "metering_ab", "frame": "%dx%d" % SIZE, "copy_line_tb_per_s": COPY_LINE_TBS, "one_frame_kernel_trace": "not measured"}
    if args[1] != "-":
        rows = list(csv.DictReader(open(args[1])))
        hist = [r for r in rows if "frame_meter_kernel" in r["Kernel_Name"]]
        summ = [r for r in rows if "frame_meter_sum_kernel" in r["Kernel_Name"]]
        hist.sort(key=lambda r: int(r["Start_Timestamp"]))
        summ.sort(key=lambda r: int(r["Start_Timestamp"]))
        assert len(hist) == len(summ) == sum(c["calls"] for c in order), (len(hist), len(summ))
        at, cases = 0, []
        for c in order:
            h = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hist[at:at + c["calls"]]]
            s = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in summ[at:at + c["calls"]]]
            at += c["calls"]
            hm = float(np.median(h))
            cases.append(dict(c, hist_us_median=round(hm, 3), hist_us_min=round(min(h), 3), sum_us_median=round(float(np.median(s)), 3),
                              hist_tb_per_s=round(c["bytes_read"] / (hm * 1e-6) / 1e12, 4), fraction_of_copy_line=round(c["bytes_read"] / (hm * 1e-6) / 1e12 / COPY_LINE_TBS, 4)))
        by = {(c["domain"], c["merge"], c["step"], c["frame"]): c for c in cases}
        for c in cases:
            c["ratio_to_random"] = round(c["hist_us_median"] / by[(c["domain"], c["merge"], c["step"], "random")]["hist_us_median"], 3)
        res["one_frame_kernel_trace"] = dict(tool="rocprofv3 --kernel-trace, a run of its own (scripts/metering_ab.py kernel)", cases=cases)
    for key, a in (("batch_128_frames", 2), ("time", 3)):
        res[key] = json.load(open(args[a])) if args[a] != "-" else "not measured"
    res["bench_py_against_the_parent_library"] = [l.rstrip("\n") for l in open(args[4]) if l.strip()] if args[4] != "-" else "not measured"
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 5:
        open(args[5], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[0] if argv else "time"
    {"kernel": cmd_kernel, "batch": cmd_batch, "time": cmd_time, "merge": cmd_merge}[mode](argv[1:])
