"""Tiled search against what there was before it, at 1280 x 1024, window and net 640 x 512, a 3 x 3 grid (overlap 128), in one
process (include/irmv_hip.h, irmv_engine_submit_tiles).

    python3 scripts/tiles_ab.py time [out.json]   cases alternated per round, 12 rounds x 50 searches each, HWC and GRBG:
                                                  (a) one tiled step: submit_tiles + wait_slots + tile_results;
                                                  (b) nine set_window + detect() calls on one slot, the host loop it replaces
                                                      (no de-duplication of the nine lists is counted);
                                                  (c) one frame-view detect(), the search at half the resolution;
                                                  and the merge alone (irmv_engine_merge_tiles: wait, merge kernel, 4 KB D2H,
                                                  synchronize -- on a zero-copy engine also the records' H2D) on the 3 x 3
                                                  step's own lists and at capacity, 16 tiles x 256 records
    python3 scripts/tiles_ab.py merge <time.json> <lines.txt> [out.json]
                                                  scripts/ab_lib.sh's lines of an alternated bench.py run against the parent's
                                                  library, merged into the JSON as they are

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL, WIN, NET, OVERLAP = (1280, 1024), (640, 512), (640, 512), 128
ROUNDS, PER_ROUND = 12, 50


def _engine(fmt, **kw):
    from irmv_detection_amd import weights
    from irmv_detection_amd.engine import YoloEngine
    extra = {} if fmt == "HWC" else dict(src_format=fmt)
    return YoloEngine(None, FULL, weights_blob=weights.synthetic_blob(0), net_size=NET[0], net_height=NET[1], window=WIN, **extra, **kw)


def _frame(fmt, i=0):
    from irmv_detection_amd import bayer, frames
    f = frames.synthetic_frame(i % 8)
    return f if fmt == "HWC" else bayer.mosaic(f, fmt)


def _stats(v):
    import numpy as np
    return dict(n=len(v), median=round(float(np.median(v)), 4), p99=round(float(np.percentile(v, 99)), 4), min=round(float(min(v)), 4))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(fmt):
    frame = _frame(fmt)
    t, one = _engine(fmt, num_slots=10), _engine(fmt)
    corners, nx, ny = t.tile_grid(OVERLAP)
    assert (nx, ny) == (3, 3)
    t.set_tiles(corners, first=1)
    t.get_src_image_buffer(0)[:] = frame
    one.get_src_image_buffer()[:] = frame
    one.set_view("frame")               # (the lazy build, paid here)
    one.set_view("window")

    def tiled():
        t.submit_tiles(0, 1, 9)
        t.wait_slots(1, 9)
        t.tile_results_raw(1)

    def host_loop():
        for x, y in corners:
            one.set_window(x, y)
            one.detect()

    def frame_view():
        one.detect()

    cases = {"a_tiled_step": tiled, "b_nine_window_detects": host_loop, "c_frame_view_detect": frame_view}
    ms = {k: [] for k in cases}
    for warm in (True, False):
        for _ in range(2 if warm else ROUNDS):
            for k, run in cases.items():
                one.set_view("frame" if k.startswith("c_") else "window")
                for _ in range(20 if warm else PER_ROUND):
                    v = _timed(run)
                    if not warm:
                        ms[k].append(v)
    one.set_view("window")
    res = {"search_ms": {k: _stats(v) for k, v in ms.items()}}
    med = {k: res["search_ms"][k]["median"] for k in cases}
    res["search_ms"]["a_over_b"] = round(med["a_tiled_step"] / med["b_nine_window_detects"], 4)
    tiled()
    recs, n_in = t.tile_results_raw(1)
    res["merge_alone_ms"] = {"typical": dict(_stats([_timed(lambda: t.merge_tiles(1, 9)) for _ in range(200)]), records_in=n_in, kept=len(recs))}
    res["graphs_held"] = t.debug_graph_count()
    t.close()
    one.close()
    return res


def merge_at_capacity():
    """16 tiles x max_det 256, every list full: 256 anchors of level 0 lit per tile, boxes one stride wide that touch."""
    import numpy as np
    e = _engine("HWC", num_slots=16, max_det=256)
    corners = (e.tile_grid(OVERLAP)[0] * 2)[:16]     # the 3 x 3 grid, walked twice: 16 tiles, every box seen by several
    e.set_tiles(corners)
    A, no = e.num_anchors, e.head_channels
    nc = no - 72
    rng = np.random.default_rng(3)
    for s in range(16):
        h = np.zeros((A, no), np.float32)
        h[:, :64] = -100.0
        h[:, 0:64:16] = 0.0
        h[:, 1:64:16] = 0.0
        h[:, 64:64 + nc] = -20.0
        lit = rng.choice(5120, 256, replace=False)
        h[lit, 64 + s % 2] = rng.uniform(0.5, 3.0, 256).astype(np.float32)
        e.write_head(h, s)
    e.run_post(0, 16)
    ms = [_timed(lambda: e.merge_tiles(0, 16)) for _ in range(200)]
    recs, n_in = e.tile_results_raw(0)
    e.close()
    return dict(_stats(ms), records_in=n_in, kept=len(recs))


def cmd_time(args):
    res = {"metric": "tiles_ab", "full": "%dx%d" % FULL, "window": "%dx%d" % WIN, "net": "%dx%d" % NET, "grid": "3x3", "overlap": OVERLAP}
    for fmt in ("HWC", "GRBG"):
        res[fmt] = measure(fmt)
    res["merge_alone_ms_at_capacity"] = merge_at_capacity()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args:
        open(args[0], "w").write(txt + "\n")


def cmd_merge(args):
    res = json.load(open(args[0]))
    res["bench_py_against_the_parent_library"] = [l.rstrip("\n") for l in open(args[1]) if l.strip()]
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(args) > 2:
        open(args[2], "w").write(txt + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    mode = argv[0] if argv else "time"
    {"time": cmd_time, "merge": cmd_merge}[mode](argv[1:])
