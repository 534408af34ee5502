"""Debug images at 1280 x 1024 with 8 detections: irmv_engine_render against the only route there was to the same picture --
get_rotated_image() (a full-size read-back) plus host gray, threshold and drawing (irmv_detection_amd/render.py, numpy).

    python3 scripts/render_ab.py time [out.json]   per (kind, scale): ALTERNATIONS rounds, each GPU_CALLS timed render() calls
                                                   then HOST_CALLS of the host route, a host clock around the synchronizing
                                                   call; and the colour, scale 1, no-marks call -- the bytes of
                                                   irmv_engine_rotated_image -- alternated with that call: its median against
                                                   the other's, and the other's own spread (max - min of its round medians)
    python3 scripts/render_ab.py kernel            20 calls per (kind, scale) and nothing else: the program of a
                                                   `rocprofv3 --kernel-trace --stats` run of its own
    python3 scripts/render_ab.py merge <time.json> <kernel_stats.csv | -> <ab_lib lines | -> [out.json]
                                                   the kernel rows of that run and scripts/ab_lib.sh's lines, merged as they are
                                                   ("-": not measured)

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
ALTERNATIONS, GPU_CALLS, HOST_CALLS = 5, 40, 4
KINDS, SCALES = ("color", "binary"), (1, 2, 4)


def _engine():
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    e = YoloEngine(None, SIZE, weights_blob=weights.synthetic_blob(0))
    e.get_src_image_buffer()[:] = frames.synthetic_frame(0)
    return e


def _dets():
    """8 detections spread over the frame: box, class and four points each."""
    import ctypes as C
    from irmv_detection_amd import capi
    out = []
    for i in range(8):
        x, y, w, h = 90.0 + 140.0 * i, 120.0 + 95.0 * i, 120.0 + 6 * i, 70.0 + 4 * i
        d = capi.Det()
        d.xyxy = (C.c_float * 4)(x, y, x + w, y + h)
        d.kpts = (C.c_float * 8)(x + 8, y + h - 6, x + 10, y + 5, x + w - 9, y + 7, x + w - 6, y + h - 4)
        d.class_id, d.armor_valid = (i * 3) % 14, 1
        out.append(d)
    return out


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    import numpy as np
    return dict(calls=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4), min=round(float(min(v)), 4))


def cmd_time(args):
    import numpy as np
    from irmv_detection_amd import render
    e, dets = _engine(), _dets()
    res = {"metric": "render_ab", "frame": "%dx%d" % SIZE, "detections": len(dets), "alternations": ALTERNATIONS, "cases": {}}
    for _ in range(20):
        e.get_rotated_image()
        e.render("color", 1, 7, dets)
    for kind in KINDS:
        for s in SCALES:
            gpu, host = [], []
            same = bool(np.array_equal(e.render(kind, s, 7, dets), render.render(e.get_rotated_image(), kind, s, 7, dets)))
            for _ in range(ALTERNATIONS):
                gpu += [_ms(lambda: e.render(kind, s, 7, dets)) for _ in range(GPU_CALLS)]
                host += [_ms(lambda: render.render(e.get_rotated_image(), kind, s, 7, dets)) for _ in range(HOST_CALLS)]
            res["cases"]["%s_s%d" % (kind, s)] = dict(render_ms=_stats(gpu), rotated_image_plus_host_drawing_ms=_stats(host),
                                                       bytes_over_pcie=(SIZE[0] // s) * (SIZE[1] // s) * 3, equal_to_the_host_reference=same)
    # the same bytes as irmv_engine_rotated_image
    rot, ren = [], []
    for _ in range(ALTERNATIONS + 1):
        rot.append([_ms(e.get_rotated_image) for _ in range(GPU_CALLS)])
        ren.append([_ms(lambda: e.render("color", 1, 0, [])) for _ in range(GPU_CALLS)])
    rot_med = [float(np.median(v)) for v in rot]
    spread = max(rot_med) - min(rot_med)
    m_rot, m_ren = float(np.median(np.concatenate(rot))), float(np.median(np.concatenate(ren)))
    res["same_bytes_as_rotated_image"] = dict(rotated_image_ms=_stats(list(np.concatenate(rot))), render_color_s1_no_marks_ms=_stats(list(np.concatenate(ren))),
                                              rotated_image_round_medians=[round(v, 4) for v in rot_med], rotated_image_spread_ms=round(spread, 4),
                                              render_minus_rotated_ms=round(m_ren - m_rot, 4), within_spread=bool(m_ren - m_rot <= spread))
    e.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def cmd_kernel(args):
    e, dets = _engine(), _dets()
    for kind in KINDS:
        for s in SCALES:
            for _ in range(20):
                e.render(kind, s, 7, dets)
    e.close()


def cmd_merge(args):
    res = json.load(open(args[0]))
    res["kernel_trace"] = "not measured"
    if args[1] != "-":
        rows = [r for r in csv.DictReader(open(args[1])) if "render_view" in r.get("Name", "") or "rotate180" in r.get("Name", "")]
        res["kernel_trace"] = dict(tool="rocprofv3 --kernel-trace --stats, a run of its own (scripts/render_ab.py kernel)", rows=rows)
    res["bench_py_against_the_parent_library"] = "not measured"
    if args[2] != "-":
        res["bench_py_against_the_parent_library"] = [l.rstrip("\n") for l in open(args[2]) if l.strip()]
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 3:
        open(args[3], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[0] if argv else "time"
    {"time": cmd_time, "kernel": cmd_kernel, "merge": cmd_merge}[mode](argv[1:])
