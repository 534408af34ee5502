"""No output of a step depends on what LDS held when its kernels started.

LDS keeps its contents from one kernel to the next.  A kernel that reads a word its workgroup has not written -- a halo
one row too wide, a padded column, an out-of-tile lane -- gets what the previous workgroup on that CU left there, and in
a test suite that is nearly always the same kernel's own earlier data: finite, plausible activations.  Such a bug passes
every bitwise test and shows up next to other work.  Here the residue is chosen (test hooks irmv_debug_lds_fill /
irmv_debug_lds_probe, csrc/k_debug.hip): before every step every LDS word of every CU is set to

    0x00000000     zeros
    0x7e007e00     two fp16 quiet NaNs: anything accumulated from it is NaN
    0xfbfffbff     two fp16 -65504: turns a max-pool, a compare or a stray accumulate visibly wrong

and everything a step leaves -- every activation tensor (read_tap), the head, the candidate count, the detections with
their poses, the classical extraction's armors -- must be the same bits under all three.

  * premise: fill(P) followed by probe(P) finds P in every word of every workgroup (share 1.0): LDS does persist across
    launches on this runtime, and the fill reaches every CU;
  * control: the probe's second output is one LDS word it never wrote; it differs between the three fills -- the bug
    class is visible to this method;
  * the engines: 1280 x 1024 -> 640 x 640 with 1 and 128 slots, 640 x 512 (tests/test_gpu_rect.py), the ShuffleNet / 416
    engine, a classical engine on rm_test.jpg, and single-slot / six-slot engines under the switches that select the
    single-frame kernels, each in both launch forms of detect() (IRMV_SYNC_LAUNCH = graph, eager);
  * reach: the profile lists of those runs together name every kernel family that uses LDS.
"""
import ctypes as C
import hashlib
import json
import os
import time

import numpy as np
import pytest

from conftest import golden_path
from irmv_detection_amd import arch, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine

pytestmark = pytest.mark.gpu

FILLS = (0x00000000, 0x7e007e00, 0xfbfffbff)
P5_C = 128


# ---- premise and control ----------------------------------------------------------------------------------------------
def _cus(rec):
    """Distinct (XCC, SE, SH, CU) the probe's workgroups ran on: HW_ID bits [15:8] and XCC_ID bits [3:0]."""
    return len({(int(x) & 0xF, (int(h) >> 8) & 0xFF) for h, x in zip(rec[:, 2], rec[:, 3])})


@pytest.mark.parametrize("pattern", [0x7e007e00, 0xfbfffbff, 0x13579bdf])
def test_premise_lds_keeps_the_fill_until_the_next_launch(pattern, capsys):
    capi.debug_lds_fill(pattern)
    rec = capi.debug_lds_probe(pattern, 0)
    other = capi.debug_lds_probe(pattern ^ 0xFFFFFFFF, 0)     # (the probe writes no LDS: the fill is still there)
    share = float(rec[:, 0].astype(np.float64).sum() / (len(rec) * capi.DEBUG_LDS_WORDS))
    with capsys.disabled():
        print(f"\n[lds residue] fill {pattern:#010x}: {len(rec)} workgroups on {_cus(rec)} distinct CUs, share of words still "
              f"holding the pattern {share:.6f} (worst workgroup {int(rec[:, 0].min())} of {capi.DEBUG_LDS_WORDS})")
    assert len(rec) >= 4 and _cus(rec) * 4 == len(rec)          # four workgroups per CU were launched: every CU was probed
    assert (rec[:, 0] == capi.DEBUG_LDS_WORDS).all(), share
    assert (other[:, 0] == 0).all()
    assert (rec[:, 1] == pattern).all()


def test_control_an_unwritten_lds_word_in_an_output_differs_between_fills():
    seen = []
    for p in FILLS:
        capi.debug_lds_fill(p)
        rec = capi.debug_lds_probe(p, 12345)
        assert (rec[:, 1] == p).all()
        seen.append(rec[:, 1].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])


# ---- the engines --------------------------------------------------------------------------------------------------------
def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def _tensors(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_ops(e._h, None, 0, C.byref(n)))
    ops = (capi.GraphOp * n.value)()
    capi.check(e._L.irmv_engine_ops(e._h, ops, n.value, C.byref(n)))
    return sorted({o.out_tensor.decode() for o in ops if o.out_tensor})


def _results_bytes(e, slot):
    n = C.c_int(0)
    dets = (capi.Det * e.max_det)()
    capi.check(e._L.irmv_engine_results(e._h, slot, dets, e.max_det, C.byref(n)))
    return n.value, bytes(dets)[:n.value * C.sizeof(capi.Det)]


def _snapshot(e, slots, tap_slots, taps, boxes):
    """{name: digest} of everything the last step left.  Heads, candidates and detections first: read_tap may re-run layers."""
    out = {}
    for s in slots:
        out[f"head[{s}]"] = _digest(e.read_head(s))
        raw = e.read_raw(s)
        out[f"candidates[{s}]"] = (raw["n_candidates"], raw["num_dets"])
        for k in ("boxes", "scores", "classes", "anchors", "kpts"):
            out[f"raw.{k}[{s}]"] = _digest(raw[k])
        out[f"detections[{s}]"] = _results_bytes(e, s)
    if boxes is not None:
        out["extract_armors"] = bytes(e.extract_armors_raw(boxes, 0))
    for s in tap_slots:
        for t in taps:
            out[f"tap {t}[{s}]"] = _digest(e.read_tap(t, s))
    return out


def _step(e, pattern, first, count):
    capi.debug_lds_fill(pattern)
    if count == 1:
        e._detect_raw(first)
    else:
        e.submit(first, count)
        e.wait()


def _residue_run(make, n_slots, images, boxes=None):
    """One engine: the batched step (engines of several slots) and detect() on the last slot, each under the three fills.
    -> (names of differing items, profile names, seconds)."""
    t0 = time.time()
    differ, names = [], set()
    with make() as e:
        for s in range(n_slots):
            e.get_src_image_buffer(s)[:] = images[s % len(images)]
        taps = _tensors(e)
        all_slots = list(range(n_slots))
        tap_slots = sorted({0, n_slots - 1, (n_slots - 1) // 2})
        steps = [(0, n_slots, all_slots, tap_slots)] if n_slots > 1 else []
        steps.append((n_slots - 1, 1, [n_slots - 1], [n_slots - 1]))
        for first, count, slots, tslots in steps:
            snaps = []
            for p in FILLS:
                _step(e, p, first, count)
                snaps.append(_snapshot(e, slots, tslots, taps, boxes))
            assert len(snaps[0]) > len(taps)
            for k, v in snaps[0].items():
                if snaps[1][k] != v or snaps[2][k] != v:
                    differ.append(f"{k} (step of {count})")
            names |= {st["name"] for st in e.profile(first, count)}
        H, W = e.net_height // 32, e.net_width // 32
        for count in {n for _, n, _, _ in steps}:
            share = -(-count // e.num_streams) if count > 1 else 1
            if "sppf_pool" in names and capi.load().irmv_sppf_slab(share, H, W, P5_C) > 0:
                names.add("sppf_pool:lds")
        form = e.sync_launch
    return differ, names, form, time.time() - t0


def _images(n, first=3):
    return [frames.synthetic_frame(first + i) for i in range(n)]


def _shuffle_blob():
    return weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)


# (id, blob, engine keywords, slots, environment, frames, classical boxes)
CONFIGS = [
    ("640x1", "yolo", dict(), 1, {}, "synthetic", False),
    ("640x128", "yolo", dict(), 128, {}, "synthetic", False),
    ("640x512x2", "yolo", dict(net_size=640, net_height=512), 2, {}, "synthetic", False),
    ("shufflenet-416x1", "shuffle", dict(net_size=416), 1, {}, "synthetic", False),
    ("classical-rm_test", "yolo", dict(point_source=capi.POINTS_CLASSICAL, rotate180=False, armor_size=capi.ARMOR_LARGE), 1, {}, "rm_test", True),
    ("640x1-single-frame-kernels", "yolo", dict(), 1,
     {"IRMV_BNECK64": "1", "IRMV_GROUP_HEAD": "1", "IRMV_GROUP_FORCE": "1", "IRMV_FORCE_PW": "1"}, "synthetic", False),
    ("640x6-kpt3", "yolo", dict(), 6, {"IRMV_KPT3": "1"}, "synthetic", False),
    ("640x1-scan-kernel", "yolo", dict(), 1, {"IRMV_EMIT_SCAN": "0"}, "synthetic", False),
]
FORMS = ("graph", "eager")
# the kernel families with LDS, as irmv_engine_profile names their launches
FAMILIES = {
    "front_kernel": lambda n: n == "front_fused",
    "c2f2_kernel": lambda n: n == "c2f2_fused",
    "c2f32_kernel": lambda n: n.startswith("c2f32_"),
    "bneck64_kernel": lambda n: n.startswith("bneck64_"),
    "kpt3_kernel": lambda n: n.startswith("kpt3_c"),
    "conv3x3_lds_kernel": lambda n: n.startswith("conv3x3s") and ("_lds_" in n or "_wres" in n),
    "conv3x3_lds_multi": lambda n: n.startswith("head_s") and "_lds" in n,
    "conv1x1_pw_kernel": lambda n: n.startswith("conv1x1s1_pw"),
    "sppf_pool_lds_kernel": lambda n: n == "sppf_pool:lds",
    "scan_decode_kernel": lambda n: n == "scan_decode",
    "nms_pnp_kernel": lambda n: n == "nms_pnp",
    "light_extract_kernel": lambda n: n == "light_extract",
}


@pytest.fixture(scope="module")
def runs(blob, rm_test_image):
    """Every configuration in both launch forms, run once for the whole module: {(id, form): (differ, names, form, s)}."""
    saved = {k: os.environ.get(k) for k in {k for c in CONFIGS for k in c[4]} | {"IRMV_SYNC_LAUNCH"}}
    blobs = {"yolo": blob, "shuffle": _shuffle_blob()}
    synthetic = _images(9)
    cases = json.load(open(golden_path("light_cases.json")))
    boxes = np.array([c["box"] for c in cases], np.float32)
    out = {}
    try:
        for tag, bk, kw, slots, env, src, classical in CONFIGS:
            for form in FORMS:
                for k in saved:
                    os.environ.pop(k, None)
                os.environ.update(env)
                os.environ["IRMV_SYNC_LAUNCH"] = form
                make = lambda: YoloEngine(None, (1280, 1024), weights_blob=blobs[bk], num_slots=slots, **kw)   # noqa: E731
                out[(tag, form)] = _residue_run(make, slots, [rm_test_image] if src == "rm_test" else synthetic, boxes if classical else None)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", [c[0] for c in CONFIGS])
def test_outputs_do_not_depend_on_the_lds_residue(runs, tag, form, capsys):
    differ, names, got_form, secs = runs[(tag, form)]
    with capsys.disabled():
        print(f"\n[lds residue] {tag} ({form}): {len(differ)} items differ between the fills; {len(names)} kernel names; {secs:.1f} s")
    assert got_form == form
    assert not differ, differ[:20]


def test_every_kernel_family_with_lds_was_reached(runs, capsys):
    names = set().union(*(r[1] for r in runs.values()))
    reached = {fam: sorted(n for n in names if match(n)) for fam, match in FAMILIES.items()}
    with capsys.disabled():
        print("\n[lds residue] reached: " + "; ".join(f"{fam}: {', '.join(v) or '-'}" for fam, v in reached.items()))
    assert all(reached.values()), [fam for fam, v in reached.items() if not v]
