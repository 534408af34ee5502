"""Tracking window against the whole frame at 1280 x 1024, in one process (include/irmv_hip.h, irmv_engine_cfg.win_width).

    python3 scripts/window_ab.py time [out.json]     detect() one frame at a time, median and p99, three engines alternated:
                                                     (a) full frame 1280 x 1024 -> 640 x 512, (b) a 640 x 512 window at 1 : 1 whose
                                                     crop reads the pinned slot, (c) the same with IRMV_WINDOW_UPLOAD=0 (upload the
                                                     frame, crop from HBM); then three single-slot async submits in flight (the
                                                     TripleBuffer shape), window engine against full-frame engine, FPS
    python3 scripts/window_ab.py kernel device       window_crop launches of 128 frames and of one frame out of the device frames,
    python3 scripts/window_ab.py kernel pinned       ... and of one frame out of the pinned slot: each for a run of its own under
                                                     `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 scripts/window_ab.py kernel ...`
    python3 scripts/window_ab.py report <device_trace.csv> <pinned_trace.csv> <time.json> [out.json]
                                                     the crop's kernel time as bytes moved over time, merged into one JSON

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL, WIN, NET = (1280, 1024), (640, 512), (640, 512)
HBM_ACHIEVABLE = 6.29e12   # float4 copy, measured
PCIE_SPEC = 63e9           # PCIe Gen5 x16


def _engine(kind, **kw):
    """kind: "full" (no window), "pinned" (window, the default upload form), "device" (window, IRMV_WINDOW_UPLOAD=0)."""
    from irmv_detection_amd import weights
    from irmv_detection_amd.engine import YoloEngine
    blob = weights.synthetic_blob(0)
    if kind == "device":
        os.environ["IRMV_WINDOW_UPLOAD"] = "0"      # (read at creation)
    try:
        return YoloEngine(None, FULL, weights_blob=blob, net_size=NET[0], net_height=NET[1], window=None if kind == "full" else WIN, **kw)
    finally:
        os.environ.pop("IRMV_WINDOW_UPLOAD", None)


def _fill(e, slots):
    from irmv_detection_amd import frames
    for s in range(slots):
        e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s % 8)


def cmd_time(args):
    import numpy as np
    res = {"metric": "window_ab", "full": "%dx%d" % FULL, "window": "%dx%d" % WIN, "net": "%dx%d" % NET}
    # ---- detect() one frame at a time: 12 rounds x 200 frames per engine after warm-up, engines alternated per round
    kinds = ["full", "pinned", "device"]
    engs = {k: _engine(k, num_slots=1) for k in kinds}
    for e in engs.values():
        _fill(e, 1)
        for _ in range(100):
            e.detect()
    ms = {k: [] for k in kinds}
    for _ in range(12):
        for k, e in engs.items():
            for i in range(200):
                if k != "full" and i % 20 == 0:
                    e.set_window_center(640 + 13 * (i // 20), 512 - 7 * (i // 20))     # the window moves, nothing is re-captured
                t0 = time.perf_counter()
                e.detect()
                ms[k].append((time.perf_counter() - t0) * 1e3)
    res["detect_ms"] = {k: dict(frames=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4),
                                min=round(float(min(v)), 4), sync_launch=engs[k].sync_launch) for k, v in ms.items()}
    prof = {}
    for k, e in engs.items():
        runs = [e.profile(0, 1) for _ in range(4)][1:]
        prof[k] = dict(launches=len(runs[0]), kernel_ms=round(sum(st["ms"] for r in runs for st in r) / len(runs), 4))
        crop = [st["ms"] for r in runs for st in r if st["name"] == "window_crop"]
        if crop:
            prof[k]["window_crop_us_event_timed"] = round(1e3 * sum(crop) / len(crop), 2)
    res["profile_single_frame"] = prof
    for e in engs.values():
        e.close()
    # ---- three single-slot async submits in flight
    tri = {}
    engs = {k: _engine(k, num_slots=3) for k in ("full", "pinned")}
    for e in engs.values():
        _fill(e, 3)
        for s in range(3):
            e.detect(s)
    fps = {k: [] for k in engs}
    for _ in range(8):
        for k, e in engs.items():
            n = 600
            t0 = time.perf_counter()
            for i in range(n):
                s = i % 3
                if i >= 3:
                    e.wait_slots(s, 1)
                e.submit(s, 1, async_upload=True)
            e.wait()
            fps[k].append(n / (time.perf_counter() - t0))
    for k, v in fps.items():
        tri["window" if k == "pinned" else k] = dict(median_fps=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
    res["three_in_flight"] = tri
    for e in engs.values():
        e.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def cmd_kernel(args):
    source = args[0] if args else "device"
    if source == "device":
        e = _engine("device", num_slots=128, num_streams=1)      # one 128-frame launch of the crop per step
        _fill(e, 128)
        e.submit(0, 128, h2d=True)
        e.wait()
        for _ in range(20):
            e.submit(0, 128, h2d=False)
        e.wait()
        e.close()
    e = _engine(source, num_slots=1)
    _fill(e, 1)
    for i in range(200):
        e.set_window(13 * (i % 40), 11 * (i % 40))               # every alignment of the source rows
        e.detect()                                                # device: upload_frame_kernel, then the crop out of HBM
    e.close()
    print("kernel probe done (%s)" % source)


def cmd_report(args):
    import csv
    import numpy as np
    dev_csv, pin_csv, time_json = args[0], args[1], args[2]
    res = json.load(open(time_json)) if os.path.exists(time_json) else {}
    moved = 2 * WIN[0] * WIN[1] * 3                   # window in + window out, per frame

    def dispatches(path, needle):
        return [r for r in csv.DictReader(open(path)) if needle in r.get("Kernel_Name", "")]

    def stats(rows, frames, nbytes, line):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if int(r["Grid_Size_Y"]) == frames]
        us = us[len(us) // 10:]                        # (the first dispatches include warm-up)
        med = float(np.median(us))
        return dict(dispatches=len(us), median_us=round(med, 2), min_us=round(min(us), 2), gbs=round(nbytes / med / 1e3, 1),
                    fraction_of_line=round(nbytes / line / (med * 1e-6), 3))

    k = {}
    dev = dispatches(dev_csv, "window_crop")
    k["device_frames_128"] = stats(dev, 128, 128 * moved, HBM_ACHIEVABLE)
    k["device_frames_1"] = stats(dev, 1, moved, HBM_ACHIEVABLE)
    k["pinned_frames_1"] = stats(dispatches(pin_csv, "window_crop"), 1, moved // 2, PCIE_SPEC)   # (the link carries the window once)
    up = dispatches(dev_csv, "upload_frame")
    if up:
        k["upload_frame_kernel_full_frame"] = stats(up, 1, FULL[0] * FULL[1] * 3, PCIE_SPEC)
    k["note"] = (f"kernel-trace durations; window_crop moves {moved} bytes per frame (window in + out); device rows against the "
                 f"{HBM_ACHIEVABLE / 1e12} TB/s measured float4-copy line, pinned and upload rows (bytes crossing the link once) against "
                 f"PCIe Gen5 x16, {PCIE_SPEC / 1e9:.0f} GB/s spec")
    res["window_crop_kernel"] = k
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 3:
        open(args[3], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[0] if argv else "time"
    {"time": cmd_time, "kernel": cmd_kernel, "report": cmd_report}[mode](argv[1:])
