"""Seeded step programs on the GPU: live setters, launch forms, slot groupings, pinned hand-off and on-demand entries
interleaved as a node interleaves them, every observation compared bit for bit with a one-slot, one-stream engine R that is
used in one way only -- all attributed state set, the attributed frame written, a synchronous detect(0) (tests/step_programs.py
holds the programs and the model that attributes; DESIGN.md, "ordering contract", the rules).

Families (step_programs.FAMILIES): W, the HWC window engine of test_gpu_window.py (322 x 201, window 256 x 128, net 128 x 64,
4 slots on 2 streams, pose prior and metering on); B, a Bayer (mhc) window engine with the refined point source (322 x 202, 3
slots); C, a plain engine on a bbox-only blob with the classical point source (322 x 201, 5 slots on 2 streams,
set_extract_params live, observed through extract_armors and the rotated image as well); P, the producer contract at
1280 x 1024 / 640 on 3 slots, with and without a rotated image of the slot between the overwrite and wait_slots.  W, B and P run
on the crafted blob of test_gpu_window.py; C on a bbox-only blob with the same class shift whose boxes are all 3 DFL bins wide
per side, on six 322 x 201 cuts of tests/golden/rm_test.jpg that each hold its armor (every observed step solves its pose).

Palettes, chosen from R's own answers on synthetic frames 10 .. 21, 40 .. 47, 60 .. 65 at the four corners and in the frame
view, measured once on the GPU -- not with the CPU oracle: R is the reference of every comparison here, so the palettes are
judged on its answers -- (every one of them gives solved poses; frames 17 and 20, as Bayer frames 18 and 44, give the same 17
records wherever the window lies and were left out):
  frames    W: 10, 11, 14, 16, 21, 41 -- 100 records at every corner, the weakest kept score 0.30 .. 0.92, so the policies below
            cut into a full list;  B: 12, 13, 15, 16, 20, 21 (mosaiced GRBG);  P: 70 .. 75.
  policies  uniform 0.25 | 0.95 on class 8 (R1), the most frequent class of those frames (1527 of 8241 records) | the colour
            mask enemy(0) (R1 .. RS off) | plates alternating SMALL / LARGE by class
  corners   (0, 0), the far corner, (31, 40 | 41), (5, 37)
test_palettes_move_the_results asserts on R alone that every policy and every corner changes an observed result.
"""
import ctypes as C
import time

import numpy as np
import pytest

import detect_craft as dc
import step_programs as sp
from irmv_detection_amd import bayer, capi, tiles, weights
from irmv_detection_amd import class_policy as cp
from irmv_detection_amd.engine import YoloEngine
from conftest import golden_path
from test_gpu_window import K, frame_of, same_results, snapshot, wblob, weng  # noqa: F401  (wblob: the module's fixture)

pytestmark = pytest.mark.gpu

FRAME_SEEDS = {"W": (10, 11, 14, 16, 21, 41), "B": (12, 13, 15, 16, 20, 21), "P": (70, 71, 72, 73, 74, 75)}
# family C: 322 x 201 cuts of tests/golden/rm_test.jpg, each with the armor (lights inside x 630 .. 785, y 360 .. 420) somewhere else
C_CUTS = ((540, 280), (560, 300), (500, 260), (600, 310), (520, 330), (580, 250))
EXTRACTS = [(150, 0.1, 0.4, 40.0, (0.8, 3.2, 3.2, 5.5)), (120, 0.05, 0.5, 45.0, (0.5, 4.0, 3.0, 6.0))]
POLICIES = [cp.uniform(0.25, capi.ARMOR_SMALL), cp.policy([0.25] * 8 + [0.95] + [0.25] * 7, capi.ARMOR_SMALL), cp.enemy(0, 0.25),
            cp.policy(0.25, [capi.ARMOR_SMALL, capi.ARMOR_LARGE] * 8)]
PRIORS = [("min_err", 8.0, capi.NORMAL_UP_ROBOT), ("prior", 8.0, capi.NORMAL_UP_ROBOT), ("prior", 2.0, 0.5)]
UPS = [(0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (0.3, -0.9, 0.2)]
REFINES = [(0.5, 4.0), (0.25, 8.0)]
METERINGS = [("view", None, 1), ("view", (13, 7, 51, 33), 2)]
ISPS = [((256, 256, 256), None), ((300, 256, 420), np.minimum(255, np.arange(256) * 5 // 4).astype(np.uint8))]
MERGES = [(0.5, 2.0), (0.3, 0.0)]
BOXES = np.array([[40, 30, 120, 90], [100, 60, 260, 150], [5, 5, 317, 196], [200, 20, 300, 80]], np.float32)      # full-frame pixels
KPTS = np.array([[50, 80, 50, 40, 110, 40, 110, 80], [120, 140, 120, 70, 240, 70, 240, 140], [60, 150, 60, 50, 250, 50, 250, 150],
                 [210, 70, 210, 30, 290, 30, 290, 70]], np.float32)
FORMS = {"default": {}, "eager": {"IRMV_SYNC_LAUNCH": "eager"}, "graph": {"IRMV_SYNC_LAUNCH": "graph"}, "no_graph_upload": {"IRMV_GRAPH_UPLOAD": "0"},
         "no_window_upload": {"IRMV_WINDOW_UPLOAD": "0"}, "inline_copies": {"IRMV_INLINE_COPIES": "1"}, "no_zero_copy": {"IRMV_ZERO_COPY_RESULTS": "0"}}
LENGTH, CASES = sp.LENGTH, sp.GPU_CASES
assert tuple(FORMS) == sp.LAUNCH_FORMS

_frames = {}


def frame(fam, i):
    if (fam, i) not in _frames:
        if fam == "C":
            if "rm" not in _frames:
                from PIL import Image
                _frames["rm"] = np.asarray(Image.open(golden_path("rm_test.jpg")).convert("RGB"))
            x, y = C_CUTS[i]
            _frames[fam, i] = np.ascontiguousarray(_frames["rm"][y:y + 201, x:x + 322])
        else:
            f = frame_of(FRAME_SEEDS[fam][i], sp.FAMILIES[fam]["full"])
            _frames[fam, i] = bayer.mosaic(f, "GRBG") if sp.FAMILIES[fam]["bayer"] else f
    return _frames[fam, i]


def engine(fam, blob, slots=None, streams=None):
    f = sp.FAMILIES[fam]
    slots, streams = slots or f["slots"], f["streams"] if streams is None else streams
    if fam == "W":
        return weng(blob, num_slots=slots, num_streams=streams)
    if fam == "B":
        return weng(blob, full=f["full"], src_format="GRBG", bayer_demosaic="mhc", point_source=capi.POINTS_REFINED, num_slots=slots, num_streams=streams)
    if fam == "C":
        return YoloEngine(None, f["full"], weights_blob=blob, net_size=128, net_height=64, camera_matrix=K, point_source=capi.POINTS_CLASSICAL,
                          num_slots=slots, num_streams=streams)
    return YoloEngine(None, f["full"], weights_blob=blob, net_size=640, camera_matrix=K, num_slots=slots, num_streams=streams)


def render_dets(fam):
    """Three records for render's marks: BOXES / KPTS rows, classes 0, 8, 14."""
    out = []
    for i, cls in enumerate((0, 8, 14)):
        d = capi.Det()
        d.xyxy, d.kpts, d.class_id, d.armor_valid = (C.c_float * 4)(*BOXES[i]), (C.c_float * 8)(*KPTS[i]), cls, 1
        out.append(d)
    return out


# ---- one operation on an engine -------------------------------------------------------------------------------------------
def set_global(e, key, v):
    if key == "policy":
        e.set_class_policy(POLICIES[v])
    elif key == "colour":
        e.set_enemy_color(v)
    elif key == "prior" and v is not None:
        e.set_pose_prior(*PRIORS[v])
    elif key == "refine":
        e.set_refine(*REFINES[v])
    elif key == "metering":
        e.set_metering(None) if v is None else e.set_metering(*METERINGS[v])
    elif key == "isp" and e.src_format != capi.SRC_HWC8:
        e.set_bayer_isp(*ISPS[v])
    elif key == "merge" and e.window_size:
        e.set_tile_merge(*MERGES[v])
    elif key == "extract":
        thr, lo, hi, ang, cd = EXTRACTS[v]
        capi.check(e._L.irmv_engine_set_extract_params(e._h, thr, lo, hi, ang, (C.c_double * 4)(*cd)))


GLOBAL_KEY = {"set_class_policy": "policy", "set_enemy_color": "colour", "set_pose_prior": "prior", "set_refine": "refine", "set_metering": "metering",
              "set_bayer_isp": "isp", "set_tile_merge": "merge", "set_extract_params": "extract"}


def set_state(e, slot, state, fam):
    """Everything a state tuple of the model holds, onto slot `slot` of an idle engine."""
    view, corner, policy, colour, prior, up, refine, metering, isp, extract = state
    if e.window_size:
        e.set_view(view, slot)
        e.set_window(corner[0], corner[1], slot)
    for key, v in (("policy", policy), ("colour", colour), ("prior", prior), ("metering", metering), ("isp", isp)):
        set_global(e, key, v)
    if fam == "B":
        set_global(e, "refine", refine)
    if fam == "C":
        set_global(e, "extract", extract)
    if prior is not None:
        e.set_up(UPS[up], slot)


def switch_on(e, fam):
    """What a W program's first operations switch on (the records exist from then on, whatever is set later)."""
    if fam == "W":
        set_global(e, "prior", 0)
        set_global(e, "metering", 0)


def entry(e, fam, kind, slot, variant=None):
    """The on-demand entry on the slot; variant: the program's slot number where the call is R's (it picks render's kind)."""
    if kind == "render":
        return e.render("binary" if (slot if variant is None else variant) % 2 else "color", 2, dets=render_dets(fam), slot=slot)
    if kind == "meter":
        return e.meter("view", (9, 5, 77, 41), 2, slot)
    if kind == "rotated":
        return e.get_rotated_image(slot)
    if kind == "extract":
        return [bytes(r) for r in e.extract_armors_raw(BOXES, slot)][:len(BOXES)]
    if kind == "refine_points":
        return [bytes(r) for r in e.refine_points(BOXES, KPTS, slot)][:len(BOXES)]
    return e.read_head(slot)


def read(e, fam, slot):
    g = dict(snap=snapshot(e, slot, False), raw=[bytes(d) for d in e.results_raw(slot)])
    if fam == "W":
        g["alts"], g["stats"] = [bytes(a) for a in e.pose_alts(slot)], e.frame_stats(slot)
    return g


def execute(e, fam, program):
    """Run the program on engine e -> what its reading operations returned, in order."""
    got = []
    f = sp.FAMILIES[fam]
    for op in program:
        k = op[0]
        if k == "write":
            e.get_src_image_buffer(op[1])[:] = frame(fam, op[2])
        elif k == "set_window":
            e.set_window(op[2][0], op[2][1], op[1])
        elif k == "set_window_center":
            assert e.set_window_center(op[2][0] + f["win"][0] / 2.0, op[2][1] + f["win"][1] / 2.0, op[1]) == tuple(op[2])
        elif k == "set_view":
            e.set_view(op[2], op[1])
        elif k == "set_up":
            e.set_up(UPS[op[2]], op[1])
        elif k == "set_tiles":
            e.set_tiles(op[2], op[1])
        elif k in GLOBAL_KEY:
            set_global(e, GLOBAL_KEY[k], op[1])
        elif k == "detect":
            e.detect(op[1])
        elif k == "submit":
            e.submit(op[1], op[2], h2d=op[3], async_upload=op[4])
        elif k == "submit_tiles":
            e.submit_tiles(op[1], op[2], op[3], h2d=op[4], async_upload=op[5])
        elif k == "run_post":
            e.run_post(op[1], 1)
        elif k == "wait":
            e.wait()
        elif k == "wait_slots":
            e.wait_slots(op[1], op[2])
        elif k == "wait_upload":
            e.wait_upload(op[1], op[2])
        elif k in sp.ENTRY_KINDS:
            got.append(entry(e, fam, k, op[1]))
        elif k in ("refused_views", "refused_window"):
            if k == "refused_views":
                rc = e._L.irmv_engine_submit(e._h, op[1], op[2], capi.SUBMIT_H2D)
            else:
                rc = e._L.irmv_engine_set_window(e._h, op[1], op[2][0], op[2][1])
            assert rc == capi.ERR_ARG, op
            got.append(dict(windows=[e.window(s)[:2] for s in range(e.num_slots)], views=[e.view(s)[0] for s in range(e.num_slots)]))
        elif k == "read":
            got.append(read(e, fam, op[1]))
        elif k == "read_tiles":
            recs, n_in = e.tile_results_raw(op[1])
            got.append(dict(kept=[(r.tile, r.index, r.cut) for r in recs], dets=[bytes(r.det) for r in recs], n_in=n_in))
        else:
            raise AssertionError(op)
    return got


# ---- the reference ---------------------------------------------------------------------------------------------------------
class Ref:
    """R: one slot, one stream; one way of use; answers cached by attribution (launch forms give the same bits, so one cache
    serves every form)."""

    def __init__(self, fam, blob):
        self.fam, self.e, self.cache, self.evals = fam, engine(fam, blob, 1, 1), {}, 0
        switch_on(self.e, fam)

    def step(self, attr, post=None):
        key = ("step", attr, post)
        if key not in self.cache:
            e = self.e
            base, after = post if post else (attr, None)
            set_state(e, 0, base[1], self.fam)
            e.get_src_image_buffer(0)[:] = frame(self.fam, base[0])
            e.detect(0)
            if after is not None:
                set_state(e, 0, after, self.fam)
                e.run_post(0, 1)
            self.cache[key] = read(e, self.fam, 0)
            self.evals += 1
        return self.cache[key]

    def entry(self, kind, attr, variant):
        key = (kind, attr, variant % 2)
        if key not in self.cache:
            if kind == "read_head":
                self.cache.pop(("step", attr, None), None)
                self.step(attr)
            else:
                set_state(self.e, 0, attr[1], self.fam)
                self.e.get_src_image_buffer(0)[:] = frame(self.fam, attr[0])
            self.cache[key] = entry(self.e, self.fam, kind, 0, variant)
        return self.cache[key]


@pytest.fixture(scope="module")
def blobs(blob, wblob):  # noqa: F811
    """Per family: the crafted blob of test_gpu_window.py; C: a bbox-only blob (nk = 0) with the same class shift and every
    box 3 bins wide on each side, so that the coarse levels' boxes hold the armor of the cut."""
    c = dc.craft(weights.synthetic_blob(0, nk=0), cls=("shift", 3.0), box=("bias", dc.dfl_bias(3)))
    return {"W": wblob, "B": wblob, "P": wblob, "C": c}


@pytest.fixture(scope="module")
def refs(blobs):
    r = {fam: Ref(fam, blobs[fam]) for fam in "WBCP"}
    yield r
    for x in r.values():
        x.e.close()


def same_stats(a, b, where):
    assert a["rect"] == b["rect"] and a["domain"] == b["domain"] and a["step"] == b["step"], where
    assert np.array_equal(a["n"], b["n"]) and np.array_equal(a["hist"], b["hist"]), where


def same_out(a, b, where):
    if isinstance(a, dict):
        same_stats(a, b, where)
    elif isinstance(a, list):
        assert a == b, where
    else:
        assert a.shape == b.shape and np.array_equal(a, b), where


def check(fam, R, obs, got, where=""):
    """Every observation of the program against R at the model's attribution -> R's answers of the step observations."""
    assert len(obs) == len(got)
    f = sp.FAMILIES[fam]
    answers = []
    for (i, o), g in zip(obs, got):
        w = (where, i, o["kind"], o["slot"])
        if o["kind"] == "read":
            ref = R.step(o["res"], o["post"])
            same_results(g["snap"], ref["snap"], o["shift"], w)
            if fam == "W":
                assert g["alts"] == ref["alts"], w
                if o["stats"] is not None:
                    same_stats(g["stats"], R.step(o["stats"])["stats"], w)
            answers.append(ref)
        elif o["kind"] == "read_tiles":
            parts = [R.step(a) for a in o["parts"]]
            lists = [dict(boxes=np.array([d["xyxy"] for d in p["snap"]["dets"]], np.float32).reshape(-1, 4),
                          scores=np.array([d["score"] for d in p["snap"]["dets"]], np.float32),
                          classes=np.array([d["ints"][0] for d in p["snap"]["dets"]], int)) for p in parts]
            corners = [a[1][1] for a in o["parts"]]
            kept, trace = tiles.merge(lists, corners, f["win"], f["full"], MERGES[o["merge"]][0], MERGES[o["merge"]][1], R.e.max_det)
            assert g["n_in"] == len(trace) and g["kept"] == kept, w
            assert g["dets"] == [parts[t]["raw"][j] for t, j, _ in kept], w
        elif o["kind"] in sp.ENTRY_KINDS:
            same_out(g, R.entry(o["kind"], o["res"], o["slot"]), w)
        else:
            assert g["windows"] == [tuple(c) for c in o["windows"]] and g["views"] == o["views"], w
    return answers


def result_key(a):
    return (tuple(a["raw"]), a["snap"]["counts"])


def fresh_engine_agrees(fam, blob, S, program):
    """F: a fresh engine in the program's final state, stepped once per slot, against S's last results."""
    m = sp.Model(fam)
    m.run(program)
    with engine(fam, blob) as F:
        switch_on(F, fam)
        for s in range(m.n):
            set_state(F, s, m.state(s), fam)
            set_global(F, "merge", m.glob["merge"])
            F.get_src_image_buffer(s)[:] = frame(fam, m.pinned[s])
        for s in range(m.n):
            F.detect(s)
        for s in range(m.n):
            a, b = read(S, fam, s), read(F, fam, s)
            same_results(a["snap"], b["snap"], (0, 0), ("fresh", s))
            assert a["raw"] == b["raw"], ("fresh", s)
            if fam == "W":
                assert a["alts"] == b["alts"], ("fresh", s)
                same_stats(a["stats"], b["stats"], ("fresh", s))


def run_case(fam, blob, R, program, where, want_launch=None):
    t0 = time.time()
    obs = sp.Model(fam).run(program)
    with engine(fam, blob) as S:
        t1 = time.time()
        got = execute(S, fam, program)
        t2 = time.time()
        answers = check(fam, R, obs, got, where)
        fresh_engine_agrees(fam, blob, S, program)
        launch = S.sync_launch
        assert want_launch is None or launch == want_launch, where
    steps = answers
    solved = sum(any(d["ints"][2] == 1 for d in a["snap"]["dets"]) for a in steps)
    distinct = len({result_key(a) for a in steps})
    print(f"step program {where}: {len(program)} operations, {len(obs)} observations ({len(steps)} of steps, {solved} with a solved pose, {distinct} distinct), "
          f"sync_launch {launch}, engine {t1 - t0:.2f} s, program {t2 - t1:.2f} s, case {time.time() - t0:.2f} s, R evaluations so far {R.evals}")
    assert 2 * solved >= len(steps) > 0 and distinct >= 6, where      # not vacuous, on R's answers alone
    return obs, got


# ---- the programs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,form,seed", CASES, ids=[f"{f}-{form}-{s}" for f, form, s in CASES])
def test_program_matches_the_reference(blobs, refs, monkeypatch, fam, form, seed):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    run_case(fam, blobs[fam], refs[fam], sp.generate(fam, seed, LENGTH), f"{fam}/{form}/{seed}", form if form in ("eager", "graph") else None)


@pytest.mark.parametrize("with_rotated", [False, True], ids=["plain", "rotated_image_in_flight"])
def test_producer_contract_at_the_real_size(wblob, refs, with_rotated):  # noqa: F811
    """12 frames round robin on 3 slots: each pinned slot is overwritten right after wait_upload, while its step runs; the
    result is the old frame's.  With the slot's rotated image asked for in between: the call waits for the slot's step
    (include/irmv_hip.h), returns the NEW frame, and the step's result is still the old frame's."""
    run_case("P", wblob, refs["P"], sp.generate_p(0, with_rotated), f"P/{'rotated' if with_rotated else 'plain'}")


def test_palettes_move_the_results(refs):
    """On R alone: every policy and every corner of the palettes changes at least one result the family's programs observe."""
    for fam in "WBC":
        R = refs[fam]
        attrs = set()
        for f, form, seed in CASES:
            if f == fam:
                attrs.update(o["res"] for _, o in sp.Model(fam).run(sp.generate(fam, seed, LENGTH)) if o["kind"] == "read" and not o["post"])
        corners = sp.FAMILIES[fam]["corners"]
        moved_p, moved_c = set(), set()
        for frame_i, st in sorted(attrs, key=repr):
            here = None
            if st[2] not in moved_p:
                here = result_key(R.step((frame_i, st)))
                if any(result_key(R.step((frame_i, st[:2] + (q,) + st[3:]))) != here for q in range(sp.N_POLICY) if q != st[2]):
                    moved_p.add(st[2])
            if st[0] == "window" and st[1] in corners and st[1] not in moved_c:
                here = here or result_key(R.step((frame_i, st)))
                if result_key(R.step((frame_i, st[:1] + (corners[(corners.index(st[1]) + 1) % 4],) + st[2:]))) != here:
                    moved_c.add(st[1])
        assert moved_p == set(range(sp.N_POLICY)) and moved_c == set(corners), (fam, moved_p, moved_c)


# ---- controls: a model that breaks one rule must be caught -----------------------------------------------------------------------
def test_a_wrong_model_is_caught(wblob, refs):  # noqa: F811
    """One W program, run once; its observations checked against the contract (passes) and against four models that each
    break one rule (each must fail)."""
    program = sp.generate("W", sp.CONTROL_SEED, sp.CONTROL_LENGTH)
    with engine("W", wblob) as S:
        got = execute(S, "W", program)
    check("W", refs["W"], sp.Model("W").run(program), got, "control")
    for flag in ("late_setters", "late_frames", "sticky_groups", "current_corner"):
        wrong = sp.Model("W", **{flag: True}).run(program)
        with pytest.raises(AssertionError):
            check("W", refs["W"], wrong, got, flag)
