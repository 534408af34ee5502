"""One tiled step (scripts/tiles_ab.py's case (a)) under another build of the library and this tree's, in ONE process: an
engine per library, searches alternated in blocks of 50 over 12 rounds, each pair created in both orders.  Run it with
IRMV_TUNE_CACHE=<fresh file> so that the second engine replays the first one's tile choices and both run the same kernels.
It takes out what separate processes add to scripts/tiles_ab.py's figure; submit_median is the host's
time inside irmv_engine_submit_tiles.

    IRMV_TUNE_CACHE=/tmp/tc.txt python3 scripts/tiles_lib_ab.py <other libirmv_hip.so> [out.json]

Diagnostics only: nothing here is imported by the product path, the tests or bench.py.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import tiles_ab
from irmv_detection_amd import capi

OLD = os.path.abspath(sys.argv[1])


def engine(fmt, lib):
    capi._lib = None
    if lib == "old":
        os.environ["IRMV_LIB_PATH"] = OLD
    else:
        os.environ.pop("IRMV_LIB_PATH", None)
    e = tiles_ab._engine(fmt, num_slots=10)
    corners, nx, ny = e.tile_grid(tiles_ab.OVERLAP)
    e.set_tiles(corners, first=1)
    e.get_src_image_buffer(0)[:] = tiles_ab._frame(fmt)
    return e


def tiled(e):
    t0 = time.perf_counter()
    e.submit_tiles(0, 1, 9)
    t1 = time.perf_counter()
    e.wait_slots(1, 9)
    e.tile_results_raw(1)
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


res = {}
for fmt in ("HWC", "GRBG"):
    for order in (("old", "new"), ("new", "old")):
        engs = {l: engine(fmt, l) for l in order}
        ms = {l: [] for l in order}
        sub = {l: [] for l in order}
        for rnd in range(-2, 12):
            for l in order:
                for _ in range(50):
                    a, b = tiled(engs[l])
                    if rnd >= 0:
                        ms[l].append(a)
                        sub[l].append(b)
        for l in order:
            res["%s created %s: %s" % (fmt, "+".join(order), l)] = dict(median=round(float(np.median(ms[l])), 4), min=round(min(ms[l]), 4),
                                                                         p99=round(float(np.percentile(ms[l], 99)), 4), submit_median=round(float(np.median(sub[l])), 4))
            engs[l].close()
print(json.dumps(res, indent=1))
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write(json.dumps(res, indent=1) + "\n")
