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

Families T and D (rule 7 and the newer side records): T is W's engine on 3 streams with pose prior, metering, yaw solve, pose
covariance, patches, the seeded number model of tests/test_gpu_numbers.py and the tracker on, W's frames; D is C's engine and
cuts with yaw solve, covariance, patches and the tracker on (device records copied out).  A read also returns yaw_poses,
pose_covs, plate_patches, plate_numbers (bit for bit against R at the attribution) and the three track records: det_tracks, the
frame header and the 32-entry snapshot, bit for bit against irmv_detection_amd/tracks.py, which replays the model's fed log
(step_programs.Replay) on the observations R's step of each attributed (frame, state) reports (test_gpu_tracks.step_obs).  The
engine under test never supplies an expectation.
  palettes  sigma_px off | 0.7 | 1.5;  yaw rounds 4, tau_max 1 | rounds 2, tau_max 0.5;  patch spans 32, 54, 12 light rows |
            30, 50, 10 light rows;  numbers off | on;  tracking off | max_misses 1, match_class 1 | max_misses 2, match_class 0,
            confirm_hits 2;  camera poses identity and the translations (2, 0, 0) mm and (0, -1, 3) mm;  stamps 1 s + 10 ms a
            clock tick.
  measured  on the GPU, on R's and the host reference's answers: every T program has 22 .. 59 observations with a
            DET_MATCHED record, 18 .. 50 with a DET_STARTED one, 5 .. 8 refused, 7 .. 23 zero, 26 .. 59 distinct byte triples and
            49 .. 395 deletions over its log; over T's eight programs 5 524 matches with 0 < d2 < gate (the millimetre
            translations, and W's frames re-seen at another corner) and 448 fed frames with n_no_room >= 1 (100 records, of
            which more are solved than the table's 32 entries hold).  D: 14 .. 24 observations with a match per program,
            110 .. 216 matches with 0 < d2 < gate, never a full table (one armor a cut).  So 10 ms a tick keeps every re-seen
            armor inside the gate and max_misses of 1 and 2 delete within a phrase; no palette value had to be changed.
"""
import ctypes as C
import time

import numpy as np
import pytest

import detect_craft as dc
import step_programs as sp
from irmv_detection_amd import bayer, capi, tiles, weights
from irmv_detection_amd import tracks as T
from irmv_detection_amd import class_policy as cp
from irmv_detection_amd.engine import YoloEngine
from conftest import golden_path
from test_gpu_numbers import model as number_model
from test_gpu_tracks import step_obs
from test_gpu_window import K, frame_of, same_results, snapshot, wblob, weng  # noqa: F401  (wblob: the module's fixture)

pytestmark = pytest.mark.gpu

FRAME_SEEDS = {"W": (10, 11, 14, 16, 21, 41), "B": (12, 13, 15, 16, 20, 21), "P": (70, 71, 72, 73, 74, 75), "T": (10, 11, 14, 16, 21, 41)}
# the palettes of the newer setters (families T and D); index 0 of COVS and TRACKING is "off"
COVS = [None, 0.7, 1.5]                                                           # sigma_px
YAWS = [dict(rounds=4, tau_max=1.0), dict(rounds=2, tau_max=0.5)]
PATCHES = [dict(span=(32, 54), light_rows=12, top=7), dict(span=(30, 50), light_rows=10, top=7)]
TRACKING = [None, dict(max_misses=1, match_class=1), dict(max_misses=2, match_class=0, confirm_hits=2)]
TRACK_OPTIONS = [None] + [T.Options(**o) for o in TRACKING[1:]]
POSES = [(T.IDENTITY, t) for t in ((0.0, 0.0, 0.0), (0.002, 0.0, 0.0), (0.0, -0.001, 0.003))]     # camera poses: translations, metres
STAMP0, TICK = 1.0, 0.01                                                          # the clock: seconds at tick 0, seconds a tick


def stamp_of(k):
    """Seconds of clock tick k (a refused_feeds model's half ticks too); a slot whose stamp was never set carries 0."""
    return 0.0 if k < 0 else STAMP0 + TICK * k


TRACKED = "TD"
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
        if fam in "CD":
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
    if fam == "T":
        e = weng(blob, num_slots=slots, num_streams=streams)
        e.set_number_model(number_model())          # (no operation of a program: the model is there before set_numbers)
        return e
    if fam == "D":
        fam = "C"
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
    elif key == "yaw" and v is not None:
        e.set_yaw_solve(**YAWS[v])
    elif key == "cov" and v is not None:
        e.set_pose_cov(False) if v == 0 else e.set_pose_cov(sigma_px=COVS[v])
    elif key == "patches" and v is not None:
        e.set_patches(**PATCHES[v])
    elif key == "numbers" and v is not None:
        e.set_numbers(bool(v))
    elif key == "tracking" and v is not None:
        e.set_tracking(False) if v == 0 else e.set_tracking(**TRACKING[v])


GLOBAL_KEY = {"set_class_policy": "policy", "set_enemy_color": "colour", "set_pose_prior": "prior", "set_refine": "refine", "set_metering": "metering",
              "set_bayer_isp": "isp", "set_tile_merge": "merge", "set_extract_params": "extract", **sp.NEW_GLOBAL}


def set_state(e, slot, state, fam):
    """Everything a state tuple of the model holds, onto slot `slot` of an idle engine -- but for the tracking options: R never
    tracks (no per-frame record depends on them), and a fresh twin sets them itself."""
    view, corner, policy, colour, prior, up, refine, metering, isp, extract = state[:10]
    for key, v in zip(("yaw", "cov", "patches", "numbers"), state[10:14]):
        set_global(e, key, v)
    if e.window_size:
        e.set_view(view, slot)
        e.set_window(corner[0], corner[1], slot)
    for key, v in (("policy", policy), ("colour", colour), ("prior", prior), ("metering", metering), ("isp", isp)):
        set_global(e, key, v)
    if fam == "B":
        set_global(e, "refine", refine)
    if fam in "CD":
        set_global(e, "extract", extract)
    if prior is not None:
        e.set_up(UPS[up], slot)


def switch_on(e, fam):
    """What a program's first operations switch on (the records exist from then on, whatever is set later) -- but for the
    tracker, which only the engines under test and their fresh twins run."""
    if fam in "WT":
        set_global(e, "prior", 0)
        set_global(e, "metering", 0)
    for op in sp.FAMILIES[fam]["preamble"]:
        if op[0] in sp.NEW_GLOBAL and op[0] != "set_tracking":
            set_global(e, sp.NEW_GLOBAL[op[0]], op[1])


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


def read(e, fam, slot, tracks=False):
    g = dict(snap=snapshot(e, slot, False), raw=[bytes(d) for d in e.results_raw(slot)])
    if fam in "WT":
        g["alts"], g["stats"] = [bytes(a) for a in e.pose_alts(slot)], e.frame_stats(slot)
    if fam in TRACKED:
        g["side"] = dict(yaws=[bytes(r) for r in e.yaw_poses(slot)], covs=[bytes(r) for r in e.pose_covs(slot)],
                         patches=[bytes(r) for r in e.plate_patches(slot)])
        if fam == "T":
            g["side"]["numbers"] = [bytes(r) for r in e.plate_numbers(slot)]
        if tracks:
            frame, snap = e.tracks(slot)
            g["tracks"] = (b"".join(bytes(d) for d in e.det_tracks(slot)), bytes(frame), b"".join(bytes(t) for t in snap))
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
        elif k == "set_stamp":
            e.set_stamp(stamp_of(op[2]), op[1])
        elif k == "set_camera_pose":
            e.set_camera_pose(POSES[op[2]][0], POSES[op[2]][1], op[1])
        elif k == "reset_tracks":
            e.reset_tracks()
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
            got.append(read(e, fam, op[1], fam in TRACKED))
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
        attr = (attr[0], attr[1][:14] + (None,))        # (the tracking options: no per-frame record depends on them)
        post = post and (post[0], post[1][:14] + (None,))
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
            if self.fam in TRACKED and post is None:
                self.cache[key]["obs"] = step_obs(e, 0)             # what the host tracker is fed for a step of this attribution
            self.evals += 1
        return self.cache[key]

    def obs_of(self, frame, state):
        return self.step((frame, state))["obs"]

    def entry(self, kind, attr, variant):
        attr = (attr[0], attr[1][:14] + (None,))
        key = (kind, attr, variant % 2)
        if key not in self.cache:
            if kind == "read_head":
                obs = self.cache.pop(("step", attr, None), {}).get("obs")
                self.step(attr)
                assert obs is None or obs == self.cache["step", attr, None]["obs"]
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
    return {"W": wblob, "B": wblob, "P": wblob, "C": c, "T": wblob, "D": c}


@pytest.fixture(scope="module")
def refs(blobs):
    r = {fam: Ref(fam, blobs[fam]) for fam in "WBCPTD"}
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


def replay_of(R, log, options=TRACK_OPTIONS, poses=POSES):
    """The host reference of the tracks (irmv_detection_amd/tracks.py) on a model's log, fed what R's steps report."""
    return sp.Replay(log, R.obs_of, options, stamp_of, poses)


def check(fam, R, obs, got, where="", replay=None):
    """Every observation of the program against R at the model's attribution -> R's answers of the step observations.
    replay: the host reference on the log of the model that made `obs` (the tracked families)."""
    assert len(obs) == len(got)
    f = sp.FAMILIES[fam]
    answers = []
    for (i, o), g in zip(obs, got):
        w = (where, i, o["kind"], o["slot"])
        if o["kind"] == "read":
            ref = R.step(o["res"], o["post"])
            same_results(g["snap"], ref["snap"], o["shift"], w)
            if fam in "WT":
                assert g["alts"] == ref["alts"], w
                if o["stats"] is not None:
                    same_stats(g["stats"], R.step(o["stats"])["stats"], w)
            if fam in TRACKED:
                for name, recs in ref["side"].items():          # (a channel its setter disabled since the step: zeroed at once)
                    assert g["side"][name] == ([bytes(len(r)) for r in recs] if name in o["wiped"] else recs), (w, name)
                if o["track"] is not None:
                    want = sp.expected_tracks(replay, o["track"], len(g["raw"]))
                    for part, a, b in zip(("det_tracks", "frame", "snapshot"), g["tracks"], want):
                        assert a == b, (w, o["track"], part)
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


def fresh_tracker_agrees(fam, blob, S, m, replay):
    """F1: a fresh one-slot engine stepped synchronously through the last epoch of the log, each step under its own tracking
    options (the last one's are the program's final ones).  Its table is the one S's last fed slot shows, every byte but
    the ids, which lie apart by exactly what S's earlier epochs issued; so do the two id counters."""
    e = len(m.epochs) - 1
    log = m.resolve(e)
    last = max(i for i, r in enumerate(log) if not r[4])
    slot = m.epochs[e][last]["slot"]
    assert m.trk[slot][1] is m.epochs[e][last], "the program's close feeds every slot: the last one still shows its step"
    earlier = replay.first_id(e) - 1
    with engine(fam, blob, 1, 1) as F:
        switch_on(F, fam)
        opts = None
        for frame_i, state, k, pose, _ in log[:last + 1]:
            set_state(F, 0, state, fam)
            if state[14] != opts:
                opts = state[14]
                set_global(F, "tracking", opts)
            F.set_stamp(stamp_of(k))
            F.set_camera_pose(POSES[pose][0], POSES[pose][1])
            F.get_src_image_buffer(0)[:] = frame(fam, frame_i)
            F.detect(0)
        (ff, fs), (sf, ss) = F.tracks(0), S.tracks(slot)
    assert sf.state == 1 and sf.next_id - ff.next_id == earlier and ff.next_id - 1 == replay.result(e, last)[1].next_id - 1 - earlier, (sf.next_id, ff.next_id, earlier)
    for a, b in zip(fs, ss):
        if b.id:
            b.id -= earlier
        assert bytes(a) == bytes(b), ("fresh tracker", a.id, b.id)
    return earlier


def fresh_engine_agrees(fam, blob, S, program, replay=None):
    """F: a fresh engine in the program's final state, stepped once per slot, against S's last results.  (The tracked
    families: but for the track records, which fresh_tracker_agrees holds.)"""
    m = sp.Model(fam)
    m.run(program)
    if fam in TRACKED:
        fresh_tracker_agrees(fam, blob, S, m, replay)
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
            if fam in "WT":
                assert a["alts"] == b["alts"], ("fresh", s)
                same_stats(a["stats"], b["stats"], ("fresh", s))
            if fam in TRACKED:
                assert a["side"] == b["side"], ("fresh", s)


_facts = {}


def track_facts(fam, R, program, key):
    """What the host reference, fed R's records, says of a tracked program: the observations the model expects and the whole
    log replayed.  Nothing here comes from an engine under test.  Memoised per (family, seed): the launch forms share it."""
    if key in _facts:
        return _facts[key]
    m = sp.Model(fam)
    obs = [o for _, o in m.run(program) if o["kind"] == "read"]
    log = m.log()
    replay = replay_of(R, log)
    f = dict(replay=replay, matched=0, started=0, moved=0, no_room=0, deleted=0, triples=set(),
             refused=sum(o["track"][0] == "refused" for o in obs), zero=sum(o["track"][0] == "zero" for o in obs))
    for o in obs:
        if o["track"][0] == "fed":
            dets, frame, _ = res = replay.result(o["track"][1], o["track"][2])
            f["matched"] += any(d.state == T.DET_MATCHED for d in dets)
            f["started"] += any(d.state == T.DET_STARTED for d in dets)
            f["triples"].add(sp.pack_tracks(res))
    for e, epoch in enumerate(log):
        seen = set()
        for k, entry in enumerate(epoch):
            dets, frame, snap = replay.result(e, k)
            gate = TRACK_OPTIONS[entry[1][14]].gate
            f["moved"] += sum(d.state == T.DET_MATCHED and 0.0 < d.d2 < gate for d in dets)
            f["no_room"] += frame.n_no_room >= 1
            ids = {t.id for t in snap if t.state != T.FREE}
            f["deleted"] += len(seen - ids)
            seen = ids
    _facts[key] = f
    return f


def run_case(fam, blob, R, program, where, want_launch=None, key=None):
    t0 = time.time()
    obs = sp.Model(fam).run(program)
    facts = track_facts(fam, R, program, key or where) if fam in TRACKED else None
    tf = time.time() - t0
    with engine(fam, blob) as S:
        t1 = time.time()
        got = execute(S, fam, program)
        t2 = time.time()
        answers = check(fam, R, obs, got, where, facts and facts["replay"])
        fresh_engine_agrees(fam, blob, S, program, facts and facts["replay"])
        launch = S.sync_launch
        assert want_launch is None or launch == want_launch, where
    if facts:
        print(f"step program {where}: tracks -- fed log {[len(e) for e in facts['replay'].log]}, observations with a match {facts['matched']}, with a start "
              f"{facts['started']}, refused {facts['refused']}, zero {facts['zero']}, distinct triples {len(facts['triples'])}; over the log: matches with "
              f"0 < d2 < gate {facts['moved']}, frames without room {facts['no_room']}, deletions {facts['deleted']}; host reference {tf:.2f} s")
        # not vacuous, on the host reference's answers alone
        assert facts["matched"] >= 1 and facts["refused"] >= 1 and len(facts["triples"]) >= 6, where
        assert fam == "D" or (facts["started"] >= 1 and facts["deleted"] >= 1 and facts["zero"] >= 1), where
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


@pytest.mark.parametrize("fam,form,seed", sp.TRACK_CASES, ids=[f"{f}-{form}-{s}" for f, form, s in sp.TRACK_CASES])
def test_tracked_program_matches_the_references(blobs, refs, monkeypatch, fam, form, seed):
    """Families T and D: the per-frame records (the four newer side records among them) against R, the three track records
    against irmv_detection_amd/tracks.py replaying the model's fed log on R's records, and the closing checks."""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    run_case(fam, blobs[fam], refs[fam], sp.generate(fam, seed, LENGTH), f"{fam}/{form}/{seed}", form if form in ("eager", "graph") else None, (fam, seed))


def test_the_tracked_set_is_not_vacuous(refs):
    """Over T's cases, on the host reference fed R's records alone: a match of a moved armor (0 < d2 < gate) and a frame
    that found no room in the table."""
    moved = no_room = 0
    for seed in sorted({s for f, _, s in sp.TRACK_CASES if f == "T"}):
        f = track_facts("T", refs["T"], sp.generate("T", seed, LENGTH), ("T", seed))
        moved, no_room = moved + f["moved"], no_room + f["no_room"]
    print(f"tracked set: matches with 0 < d2 < gate {moved}, frames without room {no_room}")
    assert moved >= 1 and no_room >= 1


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
    # the newer setters, on family T: every palette entry changes the record it governs at an observed attribution ...
    R = refs["T"]
    programs = {seed: sp.generate("T", seed, LENGTH) for seed in sorted({s for f, _, s in sp.TRACK_CASES if f == "T"})}
    attrs = set()
    for p in programs.values():
        attrs.update(o["res"] for _, o in sp.Model("T").run(p) if o["kind"] == "read" and not o["post"])
    moved = set()
    for idx, name, count in ((10, "yaws", sp.N_YAW), (11, "covs", sp.N_COV), (12, "patches", sp.N_PATCHES), (13, "numbers", sp.N_NUMBERS)):
        for v in range(count):
            for frame_i, st in sorted((a for a in attrs if a[1][idx] == v), key=repr)[:8]:
                here = R.step((frame_i, st))["side"][name]
                if any(R.step((frame_i, st[:idx] + (q,) + st[idx + 1:]))["side"][name] != here for q in range(count) if q != v):
                    moved.add((name, v))
                    break
    assert moved == {("yaws", 0), ("yaws", 1), ("covs", 0), ("covs", 1), ("covs", 2), ("patches", 0), ("patches", 1), ("numbers", 0), ("numbers", 1)}, moved
    # ... and every tracking option set, every camera pose and every sigma_px (through the tracker's noise) the track records
    # of program 0: the host reference on the same log with the entry exchanged gives other bytes
    base = track_facts("T", R, programs[0], ("T", 0))["replay"]
    log = base.log

    def moves(log, **kw):
        """Does the host reference give other bytes somewhere?  (It stops at the first entry that differs.)"""
        r = replay_of(R, log, **kw)
        return any(sp.pack_tracks(r.result(e, k)) != sp.pack_tracks(base.result(e, k)) for e in range(len(log)) for k in range(len(log[e])))

    for i in (1, 2):
        assert moves(log, options=[None, TRACK_OPTIONS[3 - i], TRACK_OPTIONS[3 - i]]), ("tracking options", i)
        assert moves(log, poses=[POSES[0] if j == i else q for j, q in enumerate(POSES)]), ("camera pose", i)
    for v in range(sp.N_COV):
        other = [[(fr, st[:11] + ((v + 1) % sp.N_COV,) + st[12:], k, pose, ref) if st[11] == v else (fr, st, k, pose, ref) for fr, st, k, pose, ref in ep] for ep in log]
        assert moves(other), ("sigma_px", v)


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
    # the T control: the contract passes; the three wrong models of rule 7 and, again, the four above are each caught
    program = sp.generate("T", sp.CONTROL_SEED, sp.CONTROL_LENGTH)
    with engine("T", wblob) as S:
        got = execute(S, "T", program)
    m = sp.Model("T")
    obs = m.run(program)
    check("T", refs["T"], obs, got, "control T", replay_of(refs["T"], m.log()))
    for flag in ("tracks_by_slot", "skips_feed", "refused_feeds", "late_setters", "late_frames", "sticky_groups", "current_corner"):
        m = sp.Model("T", **{flag: True})
        wrong = m.run(program)
        with pytest.raises(AssertionError):
            check("T", refs["T"], wrong, got, flag, replay_of(refs["T"], m.log()))
