"""No output of a step depends on what device memory held before it.

Global memory keeps its contents from one step to the next, and the engine hides a read of a word no kernel of the same step
wrote first: activation tensors, frames and records start at zero (a fresh engine reads +0), and every later step finds the
previous step's finite, plausible value, usually of the same frame.  Both pass every bitwise test.  Here the residue is chosen,
as tests/test_gpu_lds_residue.py chooses the LDS residue.  Every device range of an engine carries a class ("device
memory a step may rely on"); irmv_engine_debug_fill_mem writes a pattern over every SCRATCH range and over the channels of
every activation tensor that some op declares as written -- CONST and CARRIED ranges stay as they are, an INDEX range gets 0 or
its largest valid value, so no fill can turn a stale word into an address outside a buffer:

    0x00000000     zeros
    0x7e007e00     fp16 quiet NaNs (as fp32: 4.3e37)
    0xfbfffbff     fp16 -65504 (as fp32: -2.7e36)
    0xffffffff     NaN in fp16, fp32 and fp64, -1 in every integer

and everything a step leaves -- every activation tensor (read_tap), the head, the candidate count, the detections with their
poses, pose alternatives, metering records, the merged tile list, the classical extraction's armors -- must be the same bits
under all four and on the first step of a fresh engine that was never filled.

  * engines: the configurations of the LDS module at the smallest slot counts that reach each consumer, a refined-point-source
    engine, and the HWC and Bayer window engines of tests/step_programs.py in the window view, the frame view and as a tiled
    step; the batched step and detect() on the last slot;
  * second pass: step on frames A, fill, step on frames B, against a fresh engine's step on B -- the previous step's real data
    of ANOTHER frame is what the fill replaces;
  * a) the fill reaches what it says, b) the method sees the bug class (a reader that recomputes nothing does change under the
    fill), c) every range is classified and the exempt ones are listed here by name, d) the carried invariants hold after
    every step, e) never-written pad channels stay +0, f) the runs together reach every kernel family.
"""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import detect_craft as dc
import mem_residue as mr
import step_programs as sp
from conftest import golden_path
from irmv_detection_amd import arch, bayer, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine
from test_gpu_lds_residue import FAMILIES as LDS_FAMILIES
from test_gpu_lds_residue import P5_C, _results_bytes, _snapshot, _tensors
from test_gpu_window import K

pytestmark = pytest.mark.gpu

PATTERNS = mr.PATTERNS
SINGLE = {"IRMV_BNECK64": "1", "IRMV_GROUP_HEAD": "1", "IRMV_GROUP_FORCE": "1", "IRMV_FORCE_PW": "1"}
# (id, blob, engine keywords, slots, environment, frames, classical boxes, family of tests/step_programs.py, modes)
CONFIGS = [
    ("640x1", "yolo", dict(), 1, {}, "synthetic", False, None, ("plain",)),
    ("640x6", "yolo", dict(num_streams=2), 6, {}, "synthetic", False, None, ("plain",)),
    ("640x512x2", "yolo", dict(net_size=640, net_height=512), 2, {}, "synthetic", False, None, ("plain",)),
    ("shufflenet-int8-416x1", "shuffle", dict(net_size=416), 1, {}, "synthetic", False, None, ("plain",)),
    ("classical-rm_test", "yolo", dict(point_source=capi.POINTS_CLASSICAL, rotate180=False, armor_size=capi.ARMOR_LARGE), 1, {}, "rm_test", True, None, ("plain",)),
    ("640x6-kpt3", "yolo", dict(num_streams=2), 6, {"IRMV_KPT3": "1"}, "synthetic", False, None, ("plain",)),
    ("640x1-scan-kernel", "yolo", dict(), 1, {"IRMV_EMIT_SCAN": "0"}, "synthetic", False, None, ("plain",)),
    ("640x1-single-frame-kernels", "yolo", dict(), 1, SINGLE, "synthetic", False, None, ("plain",)),
    ("refined-x2", "yolo", dict(point_source=capi.POINTS_REFINED, rotate180=False), 2, {}, "rm_test", False, None, ("plain",)),
    ("window-hwc", "craft", dict(), 4, {}, "W", False, "W", ("window", "frame", "tiles")),
    ("window-bayer-mhc", "craft", dict(), 3, {}, "B", False, "B", ("window", "tiles")),
]
BOTH_FORMS = ("640x1", "640x6", "640x512x2")
CASES = [(c[0], form) for c in CONFIGS for form in (("graph", "eager") if c[0] in BOTH_FORMS else ("graph",))]
# c) the ranges a fill never touches, by name: everything else must be ACT or SCRATCH.  Weights and biases are the names "w." /
# "b." + layer.  A new allocation of either class fails the test until it is listed here.
CONST_NAMES = {"tap_x", "tap_y", "tap_x.frame", "tap_y.frame", "win_dev", "isp_table", "cls_dev", "pnp_dev", "prior_dev", "up_dev",
               "refine_params", "tile_params", "meter_params", "render_marks", "render_font"}
CARRIED_NAMES = {"cand_counts", "cand_bits"}


def _is_weight(name):
    return name.startswith(("w.", "b."))


# ---- engines ------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cfg, form, blobs, images):
        self.tag, bk, self.kw, self.slots, self.env, self.src, self.classical, self.fam, self.modes = cfg
        self.form, self.blob, self.images = form, blobs[bk], images

    def make(self):
        if self.fam == "W":
            e = YoloEngine(None, sp.FAMILIES["W"]["full"], weights_blob=self.blob, net_size=128, net_height=64, window=sp.FAMILIES["W"]["win"],
                           camera_matrix=K, num_slots=self.slots, num_streams=sp.FAMILIES["W"]["streams"])
            e.set_pose_prior("prior", 8.0, capi.NORMAL_UP_ROBOT)
            e.set_metering("view", (13, 7, 51, 33), 2)
        elif self.fam == "B":
            e = YoloEngine(None, sp.FAMILIES["B"]["full"], weights_blob=self.blob, net_size=128, net_height=64, window=sp.FAMILIES["B"]["win"],
                           camera_matrix=K, src_format="GRBG", bayer_demosaic="mhc", point_source=capi.POINTS_REFINED, num_slots=self.slots)
        else:
            e = YoloEngine(None, (1280, 1024), weights_blob=self.blob, num_slots=self.slots, **self.kw)
        if self.fam:
            e.set_tiles(sp.FAMILIES[self.fam]["corners"][:self.slots], 0)
        return e

    def load(self, e, which):
        imgs = self.images[self.src, which]
        for s in range(self.slots):
            e.get_src_image_buffer(s)[:] = imgs[s % len(imgs)]

    def steps(self, mode):
        n = self.slots
        if mode == "tiles":
            return [("tiles", 0, n)]
        st = [("batch", 0, n)] if n > 1 else []
        return st + ([("detect", n - 1, 1)] if mode != "frame" else [])


def _set_mode(e, mode):
    if mode != "plain":
        for s in range(e.num_slots):
            e.set_view("frame" if mode == "frame" else "window", s)


def _run_step(e, step):
    kind, first, count = step
    if kind == "detect":
        e._detect_raw(first)
    elif kind == "tiles":
        e.submit_tiles(0, first, count)
        e.wait()
    else:
        e.submit(first, count)
        e.wait()


def _snap(case, e, step, taps, boxes):
    kind, first, count = step
    slots = list(range(first, first + count))
    tap_slots = sorted({slots[0], slots[-1], slots[(count - 1) // 2]})
    out = _snapshot(e, slots, tap_slots, taps, boxes)
    if case.fam == "W":
        for s in slots:
            out[f"pose_alts[{s}]"] = mr.freeze(e.pose_alts(s))
            if kind != "tiles":
                out[f"frame_stats[{s}]"] = mr.freeze(e.frame_stats(s))
    if kind == "tiles":
        recs, n_in = e.tile_results_raw(first)
        out["tile list"] = (n_in, tuple((r.tile, r.index, r.cut, bytes(r.det)) for r in recs))
    return out


def _fresh(case, mode, step, which, boxes):
    """The first step of a fresh engine that was never filled, on the same frames."""
    with case.make() as e:
        _set_mode(e, mode)
        case.load(e, which)
        _run_step(e, step)
        return _snap(case, e, step, _tensors(e), boxes)


def _diff(ref, snap, where):
    assert ref.keys() == snap.keys()
    return [f"{k} ({where})" for k, v in ref.items() if snap[k] != v]


def _residue_run(case, boxes):
    """One configuration -> dict(differ, carried, pads, names, secs, filled, allocs, n_cand)."""
    t0 = time.time()
    out = dict(differ=[], carried=[], pads=[], names=set(), n_cand=0)
    with case.make() as e:
        taps = _tensors(e)
        for mode in case.modes:
            _set_mode(e, mode)
            for step in case.steps(mode):
                where = f"{mode} {step[0]} of {step[2]}"
                ref = {w: _fresh(case, mode, step, w, boxes) for w in "AB"}
                case.load(e, "A")
                for p in PATTERNS:                                   # pass 1: the same frames under every fill
                    e.debug_fill_mem(p)
                    _run_step(e, step)
                    out["carried"] += [(where, hex(p), b) for b in mr.carried_nonzero(e)]
                    out["differ"] += _diff(ref["A"], _snap(case, e, step, taps, boxes), f"{where}, fill {p:#010x}")
                out["pads"] += [(where, "pass 1") + b for b in mr.dirty_pad_channels(e)]
                for p in PATTERNS:                                   # pass 2: A, fill, B
                    case.load(e, "A")
                    _run_step(e, step)
                    case.load(e, "B")
                    e.debug_fill_mem(p)
                    _run_step(e, step)
                    out["carried"] += [(where, hex(p), b) for b in mr.carried_nonzero(e)]
                    out["differ"] += _diff(ref["B"], _snap(case, e, step, taps, boxes), f"{where}, A -> fill {p:#010x} -> B")
                out["pads"] += [(where, "pass 2") + b for b in mr.dirty_pad_channels(e)]
                out["n_cand"] += sum(e.read_raw(s)["n_candidates"] for s in range(step[1], step[1] + step[2]))
                if step[0] == "tiles":
                    if e.tile_results_raw(step[1])[1] > 0:
                        out["names"].add("tile_merge:ran")           # (the merge is the step's last node, not a row of the profile)
                else:
                    out["names"] |= {st["name"] for st in e.profile(step[1], step[2])}
                    out["carried"] += [(where, "profile", b) for b in mr.carried_nonzero(e)]
                    share = -(-step[2] // e.num_streams) if step[2] > 1 else 1
                    if "sppf_pool" in out["names"] and capi.load().irmv_sppf_slab(share, e.net_height // 32, e.net_width // 32, P5_C) > 0:
                        out["names"].add("sppf_pool:lds")
                if case.fam == "W" and any(a.state for s in range(e.num_slots) for a in e.pose_alts(s)):
                    out["names"].add("nms_pnp<true>:ran")            # (the pose-alt instantiation keeps the profile name nms_pnp)
        out["allocs"] = e.debug_allocs()
        out["filled"] = e.debug_fill_mem(0)
        out["expect"] = mr.expected_fill_bytes(e, out["allocs"])
        out["form"] = e.sync_launch
    out["secs"] = time.time() - t0
    return out


@pytest.fixture(scope="module")
def blobs(blob):
    specs, tensors = weights.synthetic_tensors(0, arch.NUM_CLASSES, arch.NUM_KPT_CH, None, True, arch.BACKBONE_SHUFFLE)
    return {"yolo": blob, "shuffle": weights.build_blob_int8(specs, tensors, arch.NUM_CLASSES, arch.NUM_KPT_CH, arch.BACKBONE_SHUFFLE),
            "craft": dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))}


@pytest.fixture(scope="module")
def images(rm_test_image):
    W, B = sp.FAMILIES["W"]["full"], sp.FAMILIES["B"]["full"]
    syn = lambda seeds, size: [frames.synthetic_frame(i, size[0], size[1]) for i in seeds]   # noqa: E731
    return {("synthetic", "A"): syn(range(3, 9), (1280, 1024)), ("synthetic", "B"): syn(range(23, 29), (1280, 1024)),
            ("rm_test", "A"): [rm_test_image, frames.synthetic_frame(5)], ("rm_test", "B"): [frames.synthetic_frame(6), rm_test_image],
            ("W", "A"): syn((10, 11, 14, 16), W), ("W", "B"): syn((21, 41, 10, 14), W),
            ("B", "A"): [bayer.mosaic(f, "GRBG") for f in syn((12, 13, 15), B)], ("B", "B"): [bayer.mosaic(f, "GRBG") for f in syn((16, 20, 21), B)]}


@pytest.fixture(scope="module")
def runs(blobs, images):
    """Every configuration, run once for the whole module: {(id, form): _residue_run's record}."""
    saved = {k: os.environ.get(k) for k in {k for c in CONFIGS for k in c[4]} | {"IRMV_SYNC_LAUNCH"}}
    cases = json.load(open(golden_path("light_cases.json")))
    boxes = np.array([c["box"] for c in cases], np.float32)
    out = {}
    try:
        for cfg in CONFIGS:
            for tag, form in CASES:
                if tag != cfg[0]:
                    continue
                for k in saved:
                    os.environ.pop(k, None)
                os.environ.update(cfg[4])
                os.environ["IRMV_SYNC_LAUNCH"] = form
                out[(tag, form)] = _residue_run(Case(cfg, form, blobs, images), boxes if cfg[6] else None)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def _per_class(allocs):
    by = {}
    for a in allocs:
        by[a["cls"]] = by.get(a["cls"], 0) + a["bytes"]
    return by


@pytest.mark.parametrize("tag,form", CASES)
def test_outputs_do_not_depend_on_what_device_memory_held(runs, tag, form, capsys):
    r = runs[(tag, form)]
    with capsys.disabled():
        print(f"\n[mem residue] {tag} ({form}): {len(r['differ'])} items differ; {r['secs']:.1f} s; candidates seen {r['n_cand']}; filled "
              f"{r['filled']} bytes (SCRATCH {r['expect']['SCRATCH']}, ACT written {r['expect']['ACT']}); registry bytes per class "
              f"{_per_class(r['allocs'])}; kernels {sorted(r['names'])}")
    assert r["form"] == form
    assert not r["differ"], r["differ"][:20]


@pytest.mark.parametrize("tag,form", CASES)
def test_d_the_carried_ranges_are_zero_after_every_step(runs, tag, form):
    assert not runs[(tag, form)]["carried"], runs[(tag, form)]["carried"][:10]


@pytest.mark.parametrize("tag,form", CASES)
def test_e_never_written_pad_channels_stay_zero(runs, tag, form):
    assert not runs[(tag, form)]["pads"], runs[(tag, form)]["pads"][:10]


@pytest.mark.parametrize("tag,form", CASES)
def test_c_every_range_is_classified_and_the_exempt_ones_are_listed(runs, tag, form):
    r = runs[(tag, form)]
    allocs = r["allocs"]
    assert r["filled"] == r["expect"]["SCRATCH"] + r["expect"]["ACT"], (r["filled"], r["expect"])      # a) the count, computed here
    const = {a["name"] for a in allocs if a["cls"] == "CONST" and not _is_weight(a["name"])}
    carried = {a["name"] for a in allocs if a["cls"] == "CARRIED"}
    assert const <= CONST_NAMES and carried == CARRIED_NAMES, (const - CONST_NAMES, carried ^ CARRIED_NAMES)
    assert const >= {"tap_x", "tap_y", "cls_dev", "pnp_dev"}, const                                    # (what every engine has)
    assert all(a["cls"] == "CONST" for a in allocs if _is_weight(a["name"]))
    assert all(a["cls"] in capi.MEM_CLASSES and a["kind"] in capi.MEM_KINDS and a["name"] and a["bytes"] > 0 for a in allocs)
    assert all(a["kind"] != "INDEX" or a["bytes"] % 4 == 0 for a in allocs)
    # the exempt bytes, weights aside, are a sliver of the engine: tap tables (8 bytes a net column / row), tables of a few
    # hundred bytes, and A / 8 bytes of bitmap a slot against 96 A fp32 of head a slot alone
    exempt = sum(a["bytes"] for a in allocs if a["cls"] in ("CONST", "CARRIED") and not _is_weight(a["name"]))
    assert exempt < 0.01 * sum(a["bytes"] for a in allocs), (exempt, sum(a["bytes"] for a in allocs))


def test_f_every_kernel_family_was_reached(runs, capsys):
    names = set().union(*(r["names"] for r in runs.values()))
    fams = dict(LDS_FAMILIES)
    fams.update({"window_crop_kernel": lambda n: n == "window_crop", "bayer_demosaic (mhc)": lambda n: n == "bayer_demosaic_mhc",
                 "tile_merge_kernel": lambda n: n == "tile_merge:ran", "light_extract_kernel<true> (refine)": lambda n: n == "light_refine",
                 "frame_meter_kernel": lambda n: n == "frame_meter", "nms_pnp_kernel<true>": lambda n: n == "nms_pnp<true>:ran"})
    reached = {fam: sorted(n for n in names if match(n)) for fam, match in fams.items()}
    with capsys.disabled():
        print("\n[mem residue] reached: " + "; ".join(f"{fam}: {', '.join(v) or '-'}" for fam, v in reached.items()))
    assert all(reached.values()), [fam for fam, v in reached.items() if not v]
    assert sum(r["n_cand"] for r in runs.values()) > 0


# ---- a) the fill reaches what it says, b) the method sees the bug class -----------------------------------------------------
@pytest.fixture(scope="module")
def control(blobs):
    saved = os.environ.get("IRMV_SYNC_LAUNCH")
    os.environ["IRMV_SYNC_LAUNCH"] = "graph"
    try:
        with YoloEngine(None, (1280, 1024), weights_blob=blobs["craft"], num_slots=2, num_streams=1) as e:
            yield e
    finally:
        os.environ.pop("IRMV_SYNC_LAUNCH", None)
        if saved is not None:
            os.environ["IRMV_SYNC_LAUNCH"] = saved


@pytest.fixture(scope="module")
def unstepped(blobs):
    """An engine that never steps: nothing of it is stale, so no read of a tensor runs a read-back step."""
    with YoloEngine(None, (1280, 1024), weights_blob=blobs["craft"], num_slots=2, num_streams=1) as e:
        yield e


@pytest.mark.parametrize("pattern", PATTERNS[1:])
def test_a_the_fill_covers_the_written_channels_and_nothing_else(unstepped, pattern):
    e = unstepped
    written = mr.written_channels(e)
    assert set(written) >= set(_tensors(e))
    filled = e.debug_fill_mem(pattern)
    expect = mr.expected_fill_bytes(e)
    assert filled == expect["SCRATCH"] + expect["ACT"], (filled, expect)
    n_pad = 0
    for t, ch in written.items():
        bits = mr.read_tensor_bits(e, t)
        want = np.zeros(bits.shape[-1], bits.dtype)
        want[ch] = pattern & (0xffff if bits.dtype == np.uint16 else 0xffffffff)
        n_pad += bits.shape[-1] - len(ch)
        wrong = np.unique(np.argwhere(bits != want)[:, -1])
        assert not len(wrong), (t, wrong.tolist(), [hex(int(v)) for v in np.unique(bits[..., wrong])[:8]])
    assert n_pad > 0                                                  # there are pad channels, and none of them was filled
    e.debug_fill_mem(0)


def test_a_the_fill_leaves_const_and_carried_ranges_and_rejects_a_pattern_with_a_phase(control):
    e = control
    e.get_src_image_buffer(0)[:] = frames.synthetic_frame(3)
    e._detect_raw(0)
    before = _snapshot(e, [0], [0], _tensors(e), None)
    e.debug_fill_mem(0xffffffff)
    assert not mr.carried_nonzero(e)
    e._detect_raw(0)                                                  # tables, weights and taps are as they were: the same step again
    assert _snapshot(e, [0], [0], _tensors(e), None) == before
    filled = C.c_uint64(0)
    assert e._L.irmv_engine_debug_fill_mem(e._h, 0x12345678, C.byref(filled)) == capi.ERR_ARG


def test_b_a_reader_that_recomputes_nothing_sees_the_fill(control, capsys):
    """run_post reads the head and recomputes nothing: after a fill its result is another one.  Inverted by hand once (the
    assertion below as `==`): it fails, as it must."""
    e = control
    e.get_src_image_buffer(0)[:] = frames.synthetic_frame(3)
    e._detect_raw(0)
    raw = e.read_raw(0)
    step = (raw["n_candidates"], raw["num_dets"], _results_bytes(e, 0))
    assert raw["n_candidates"] > 0 and raw["num_dets"] > 0           # premise: the step found something to lose
    e.read_head(0)                                                    # (the dense head: run_post then runs no read-back step)
    e.run_post(0, 1)
    raw = e.read_raw(0)
    assert (raw["n_candidates"], raw["num_dets"], _results_bytes(e, 0)) == step   # run_post alone reproduces the step
    e.debug_fill_mem(0xffffffff)
    e.run_post(0, 1)
    raw = e.read_raw(0)
    got = (raw["n_candidates"], raw["num_dets"], _results_bytes(e, 0))
    with capsys.disabled():
        print(f"\n[mem residue] control: step {step[:2]} candidates / detections, run_post on a filled head {got[:2]}")
    assert got != step
    assert not mr.carried_nonzero(e)


def test_b_a_conv_on_a_filled_input_sees_the_fill(control):
    """One mid-network conv run alone (no poison flag) on an input the fill covered: its output is not the step's."""
    e = control
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_conv_ops(e._h, None, 0, C.byref(n)))
    ops = (capi.ConvOp * n.value)()
    capi.check(e._L.irmv_engine_conv_ops(e._h, ops, n.value, C.byref(n)))
    mid = [o for o in ops if o.ks == 3 and o.stride == 2 and not o.out_lazy and not o.fused and o.cin >= 64]
    assert mid
    o = mid[0]
    e.get_src_image_buffer(0)[:] = frames.synthetic_frame(3)
    e._detect_raw(0)
    name = o.out_tensor.decode()
    step = mr.read_tensor_bits(e, name)[0, ..., o.out_coff:o.out_coff + o.cout].copy()
    capi.check(e._L.irmv_engine_run_conv_candidate(e._h, o.op, 1, -1, 0, 1, 0))
    assert np.array_equal(mr.read_tensor_bits(e, name)[0, ..., o.out_coff:o.out_coff + o.cout], step)   # alone, on the step's input: the step's output
    e.debug_fill_mem(0x7e007e00)
    capi.check(e._L.irmv_engine_run_conv_candidate(e._h, o.op, 1, -1, 0, 1, 0))
    got = mr.read_tensor_bits(e, name)[0, ..., o.out_coff:o.out_coff + o.cout]
    assert not np.array_equal(got, step)
    e.debug_fill_mem(0)
