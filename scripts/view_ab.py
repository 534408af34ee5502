"""Search view against a second engine at 1280 x 1024, window and net 640 x 512, HWC and GRBG, in one process
(include/irmv_hip.h, irmv_engine_set_view).

    python3 scripts/view_ab.py time [out.json]    per source format, engines alternated per round, 12 rounds x 200 frames each:
                                                  detect() one frame at a time on (a) a plain full-frame engine, (a2) a second
                                                  one like it -- the run-to-run spread of (a) --, (b) the window engine in the
                                                  frame view, (c) the window engine in the window view; the loss frame -- window
                                                  detect() + set_view(frame) + detect() on the same pinned frame against window
                                                  detect() + a host copy of the frame into a second engine's slot + its
                                                  detect(); and set_view itself, first call (the lazy build) and later ones
    python3 scripts/view_ab.py window             the window engine's window-view detect() alone, one JSON line: run once per
                                                  library under IRMV_LIB_PATH to compare two builds (it never calls set_view)
    python3 scripts/view_ab.py merge <time.json> <lines.txt> [out.json]
                                                  the `window` lines and scripts/ab_lib.sh's lines of an alternated run, merged
                                                  into the JSON as they are

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL, WIN, NET = (1280, 1024), (640, 512), (640, 512)
ROUNDS, PER_ROUND = 12, 200


def _engine(fmt, window, **kw):
    from irmv_detection_amd import weights
    from irmv_detection_amd.engine import YoloEngine
    extra = {} if fmt == "HWC" else dict(src_format=fmt)
    return YoloEngine(None, FULL, weights_blob=weights.synthetic_blob(0), net_size=NET[0], net_height=NET[1],
                      window=WIN if window else None, **extra, **kw)


def _frame(fmt, i=0):
    from irmv_detection_amd import bayer, frames
    f = frames.synthetic_frame(i % 8)
    return f if fmt == "HWC" else bayer.mosaic(f, fmt)


def _stats(v):
    import numpy as np
    return dict(frames=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4), min=round(float(min(v)), 4))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(fmt):
    res = {}
    frame = _frame(fmt)
    a, a2, w = _engine(fmt, False), _engine(fmt, False), _engine(fmt, True)
    for e in (a, a2, w):
        e.get_src_image_buffer()[:] = frame
    # ---- the switch itself
    first = _timed(lambda: w.set_view("frame"))
    later = []
    for i in range(200):
        later.append(_timed(lambda: w.set_view("window" if i % 2 == 0 else "frame")))
    res["set_view_ms"] = dict(first_call_lazy_build=round(first, 3), later=_stats(later))
    # ---- detect() one frame at a time
    def in_view(view):
        def run():
            w.detect()
        return view, run
    cases = {"a_plain": (None, a.detect), "a2_plain_again": (None, a2.detect), "b_frame_view": in_view("frame"), "c_window_view": in_view("window")}
    for view, run in cases.values():
        if view:
            w.set_view(view)
        for _ in range(100):
            run()
    ms = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, (view, run) in cases.items():
            if view:
                w.set_view(view)
            for _ in range(PER_ROUND):
                ms[k].append(_timed(run))
    res["detect_ms"] = {k: _stats(v) for k, v in ms.items()}
    res["detect_ms"]["sync_launch"] = dict(plain=a.sync_launch, window_engine=w.sync_launch)
    med = {k: res["detect_ms"][k]["median"] for k in cases}
    res["detect_ms"]["spread_of_a_ms"] = round(abs(med["a_plain"] - med["a2_plain_again"]), 4)
    res["detect_ms"]["b_minus_a_ms"] = round(med["b_frame_view"] - med["a_plain"], 4)
    w.set_view("frame")
    names_a, names_b = [st["name"] for st in a.profile(0, 1)], [st["name"] for st in w.profile(0, 1)]
    w.set_view("window")
    res["launches"] = dict(a_plain=len(names_a), b_frame_view=len(names_b), b_same_kernel_names_as_a=names_a == names_b,
                           c_window_view=len(w.profile(0, 1)))
    # ---- the loss frame: the target is not in the window, the same frame is searched whole
    src_w, src_a = w.get_src_image_buffer(), a.get_src_image_buffer()
    one, two = [], []
    for _ in range(ROUNDS):
        for _ in range(PER_ROUND // 4):
            w.set_view("window")

            def one_engine():
                w.detect()
                w.set_view("frame")
                w.detect()
            one.append(_timed(one_engine))
        w.set_view("window")
        for _ in range(PER_ROUND // 4):
            def two_engines():
                w.detect()
                src_a[:] = src_w            # what a two-engine user pays: the frame into the other engine's pinned slot
                a.detect()
            two.append(_timed(two_engines))
    res["loss_frame_ms"] = dict(one_engine_set_view=_stats(one), two_engines_host_copy=_stats(two),
                                frame_bytes=int(src_w.nbytes))
    for e in (a, a2, w):
        e.close()
    return res


def cmd_time(args):
    res = {"metric": "view_ab", "full": "%dx%d" % FULL, "window": "%dx%d" % WIN, "net": "%dx%d" % NET}
    for fmt in ("HWC", "GRBG"):
        res[fmt] = measure(fmt)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def cmd_window(args):
    fmt = args[0] if args else "HWC"
    w = _engine(fmt, True)
    w.get_src_image_buffer()[:] = _frame(fmt)
    for _ in range(100):
        w.detect()
    ms = [_timed(w.detect) for _ in range(ROUNDS * PER_ROUND)]
    w.close()
    print(json.dumps(dict(window_view_detect_ms=_stats(ms), src=fmt, lib="IRMV_LIB_PATH build" if os.environ.get("IRMV_LIB_PATH") else "in-tree")))


def cmd_merge(args):
    res = json.load(open(args[0]))
    lines = [l.rstrip("\n") for l in open(args[1]) if l.strip()]
    res["against_the_parent_library"] = dict(
        window_view_detect=[json.loads(l) for l in lines if l.startswith("{")],
        bench_py=[l for l in lines if not l.startswith("{")])
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 2:
        open(args[2], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[0] if argv else "time"
    {"time": cmd_time, "window": cmd_window, "merge": cmd_merge}[mode](argv[1:])
