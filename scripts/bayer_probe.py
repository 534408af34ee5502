"""Raw Bayer input against HWC input at 1280 x 1024, in one process (include/irmv_hip.h IRMV_SRC_BAYER_*8).

    python3 scripts/bayer_probe.py time [out.json]     single-frame detect() clock and host-inclusive throughput, engines alternated
    python3 scripts/bayer_probe.py kernel              demosaic launches of 1 and 128 frames, for `rocprofv3 --kernel-trace --stats`
    python3 scripts/bayer_probe.py kernel --demosaic mhc
                                                       the same with three engines alternated in one process: Malvar-He-Cutler
                                                       (bayer_demosaic_mhc_kernel), bilinear with the gains as arguments
                                                       (bayer_demosaic_kernel) and bilinear after irmv_engine_set_bayer_isp
                                                       (bayer_demosaic_lut_kernel); `report` then lists each kernel by name
    python3 scripts/bayer_probe.py report <kernel_trace.csv> <time.json> [out.json]
                                                       the demosaic's kernel time and its fraction of the HBM line, merged into one JSON

`time` compares an IRMV_SRC_HWC8 engine with an IRMV_SRC_BAYER_RGGB8 one fed the same frames (the HWC one the demosaiced
frame).  Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

W, H = 1280, 1024
HBM_PEAK = 8.0e12        # MI355X HBM3E, spec
HBM_ACHIEVABLE = 6.29e12  # float4 copy, measured


DEMOSAIC = "bilinear"     # --demosaic mhc: the Bayer engines of `time` use the Malvar-He-Cutler kernel; `kernel` compares the three kernels


def _engines(kinds, **kw):
    """kinds: "hwc", "bayer" (DEMOSAIC), or a Bayer engine by kernel: "bilinear", "mhc", "lut" (bilinear after a set)."""
    from irmv_detection_amd import weights
    from irmv_detection_amd.engine import YoloEngine
    blob = weights.synthetic_blob(0)
    out = {}
    for k in kinds:
        algo = {"bayer": DEMOSAIC, "mhc": "mhc"}.get(k, "bilinear")
        out[k] = YoloEngine(None, (W, H), weights_blob=blob, src_format=0 if k == "hwc" else "RGGB", bayer_demosaic=algo, **kw)
        if k == "lut":
            out[k].set_bayer_isp((256, 256, 256))
    return out


def _fill(engs, slots):
    from irmv_detection_amd import bayer, frames
    raws = [bayer.mosaic(frames.synthetic_frame(i), "RGGB") for i in range(min(slots, 8))]
    hwcs = [bayer.demosaic(r, "RGGB", algo=DEMOSAIC) for r in raws] if "hwc" in engs else []
    for s in range(slots):
        for k, e in engs.items():
            e.get_src_image_buffer(s)[:] = hwcs[s % 8] if k == "hwc" else raws[s % 8]


def cmd_time(args):
    import numpy as np
    kinds = ["hwc", "bayer"]
    res = {}
    # ---- the single-frame detect() clock: 12 rounds x 200 frames per engine after warm-up, engines alternated per round
    engs = _engines(kinds, num_slots=3)
    _fill(engs, 3)
    lat = {k: [] for k in kinds}
    for k in kinds:
        for _ in range(200):
            engs[k].detect(0)
    for _ in range(12):
        for k in kinds:
            e = engs[k]
            for _ in range(200):
                t0 = time.perf_counter()
                e.detect(0)
                lat[k].append(time.perf_counter() - t0)
    res["single_frame_detect_ms"] = {k: dict(frames=len(v), median=round(float(np.median(v)) * 1e3, 4), p99=round(float(np.percentile(v, 99)) * 1e3, 4),
                                             mean=round(float(np.mean(v)) * 1e3, 4), sync_launch=engs[k].sync_launch) for k, v in lat.items()}
    for e in engs.values():
        e.close()
    # ---- host-inclusive throughput: 256 pinned slots, groups of 32 submitted with H2D | ASYNC_UPLOAD (bench.py's clock)
    B, G, steps = 256, 32, 30
    engs = _engines(["hwc", "bayer"], num_slots=B)
    _fill(engs, B)
    fps = {k: [] for k in engs}
    for rnd in range(4):
        for k, e in engs.items():
            for _ in range(2 if rnd == 0 else 0):
                for f in range(0, B, G):
                    e.submit(f, G, h2d=True, async_upload=True)
                e.wait()
            t0 = time.perf_counter()
            for _ in range(steps):
                for f in range(0, B, G):
                    e.submit(f, G, h2d=True, async_upload=True)
            e.wait()
            fps[k].append(B * steps / (time.perf_counter() - t0))
    res["host_inclusive_fps"] = {k: dict(rounds=[round(v, 1) for v in vs], median=round(float(np.median(vs)), 1),
                                         upload_gbs=round(float(np.median(vs)) * (W * H * (3 if k == "hwc" else 1)) / 1e9, 2))
                                 for k, vs in fps.items()}
    for e in engs.values():
        e.close()
    from build_stamp import build_stamp
    res["build"] = build_stamp()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        open(args[0], "w").write(txt + "\n")


def cmd_kernel(args):
    """One 128-frame launch of the demosaic per step (one compute stream), and single-frame ones."""
    if DEMOSAIC == "mhc":
        return cmd_kernel_alternated()
    e = _engines(["bayer"], num_slots=128, num_streams=1)["bayer"]
    _fill({"bayer": e}, 128)
    for _ in range(20):
        e.submit(0, 128, h2d=False)
    e.wait()
    e.close()
    e = _engines(["bayer"], num_slots=1)["bayer"]
    _fill({"bayer": e}, 1)
    for _ in range(200):
        e.submit(0, 1, h2d=False)
        e.wait()
    e.close()
    print("kernel probe done")


def cmd_kernel_alternated():
    """The three demosaic kernels in one process, their engines taking turns step by step: 20 steps of 128 frames and 200
    of one frame each (the raw frames already in the device slots)."""
    kinds = ["mhc", "bilinear", "lut"]
    for slots, steps, kw in ((128, 20, dict(num_streams=1)), (1, 200, {})):
        engs = _engines(kinds, num_slots=slots, **kw)
        _fill(engs, slots)
        for e in engs.values():
            e.submit(0, slots, h2d=True)
            e.wait()
        for _ in range(steps):
            for e in engs.values():
                e.submit(0, slots, h2d=False)
                e.wait()
        for e in engs.values():
            e.close()
    print("kernel probe done (alternated: " + ", ".join(kinds) + ")")


def cmd_report(args):
    import csv
    import numpy as np
    trace_csv, time_json = args[0], args[1]
    rows = [r for r in csv.DictReader(open(trace_csv)) if "bayer_demosaic" in r.get("Kernel_Name", "")]
    if not rows:
        raise SystemExit("no bayer_demosaic dispatches in " + trace_csv)
    res = json.load(open(time_json)) if os.path.exists(time_json) else {}
    per_frame = W * H + W * H * 3          # raw in + HWC out, once per frame (the halo rows' re-reads are not counted)
    def kernel_of(r):       # bayer_demosaic_kernel / bayer_demosaic_lut_kernel / bayer_demosaic_mhc_kernel
        n = r["Kernel_Name"]
        return "bayer_demosaic_mhc" if "demosaic_mhc" in n else ("bayer_demosaic_lut" if "demosaic_lut" in n else "bayer_demosaic")
    names = sorted({kernel_of(r) for r in rows})
    k = {}
    for name in names:
        mine = [r for r in rows if kernel_of(r) == name]
        d = {}
        for frames in sorted({int(r["Grid_Size_Y"]) for r in mine}):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine if int(r["Grid_Size_Y"]) == frames]
            med = float(np.median(us))
            d[f"frames_{frames}"] = dict(dispatches=len(us), median_us=round(med, 2), min_us=round(min(us), 2),
                                         gbs=round(frames * per_frame / med / 1e3, 1),
                                         fraction_of_hbm_peak=round(frames * per_frame / HBM_PEAK / (med * 1e-6), 3),
                                         fraction_of_hbm_achievable=round(frames * per_frame / HBM_ACHIEVABLE / (med * 1e-6), 3))
        if names == ["bayer_demosaic"]:
            k.update(d)                 # (a run of the one kernel: the layout profiles/bayer_probe.json has)
        else:
            k[name] = d
    k["note"] = (f"kernel-trace durations; bytes = {per_frame} per frame (raw in + HWC out); peak {HBM_PEAK / 1e12} TB/s spec, "
                 f"{HBM_ACHIEVABLE / 1e12} TB/s the measured float4-copy line")
    res["demosaic_kernel"] = k
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 2:
        open(args[2], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--demosaic" in argv:
        i = argv.index("--demosaic")
        DEMOSAIC = argv[i + 1]
        if DEMOSAIC not in ("bilinear", "mhc"):
            raise SystemExit("--demosaic bilinear|mhc")
        del argv[i:i + 2]
    mode = argv[0] if argv else "time"
    {"time": cmd_time, "kernel": cmd_kernel, "report": cmd_report}[mode](argv[1:])
