"""All four side-record channels alive on one engine: pose alts, constrained poses, plate patches and the metering record.

Each feature's own test file holds an engine with that ONE feature to its host reference.  Here engine ALL enables all four
(once in the order alts, yaw, patches, metering, once in the reverse order), engines ONE_x exactly one each, all see the same
frames, and every record ALL delivers must be the bytes ONE_x delivers -- so ALL stands on the same references -- in every
step form: detect(), a batched submit, run_post on a head read back from a step, a tiled step, and a window engine's frame
view built after the features were enabled.  The result records themselves must not notice any of it.

Shapes: those of tests/patch_set.py (128 x 96 source, 64 x 64 net, seeded weights, its step frames), three slots, and a
64 x 64 window engine for the tiled step and the frame view.  Three engine kinds: a keypoint engine (records written into
pinned memory), the same with IRMV_ZERO_COPY_RESULTS=0 (device records and copies) and a classical one (device records).
The pose prior is set to its defaults (MIN_ERR, every tilt 0): what an engine that never set one solves the yaw with.

The classical engine pairs light bars it finds in the frame, and the seeded step frames hold none (no test counts an armor
on them), so its frames are the step frames with one plate's two bars drawn in (tests/test_gpu_pnp.py _draw_bar) and its
binary threshold is 250, which only the bars pass.  The seeded weights' boxes cover most of the frame, so the bars lie in
nearly every record's box.  The keypoint engines see the step frames as they are.

So that equal-but-empty records cannot pass, every channel of every ONE_x engine must show a record that is not all zero in
every step form in which its feature runs.  Tiled steps and run_post do not meter: there the metering record must still be
the one of the slot's last ordinary step.
"""
import contextlib
import ctypes as C

import pytest

import patch_set as PS
import test_gpu_patches as TP
from irmv_detection_amd import capi
from test_gpu_pnp import _draw_bar

pytestmark = pytest.mark.gpu

SLOTS = 3
CORNERS = [(0, 0), (40, 20)]      # the tiles of slots 1 and 2; the first keeps result keypoints window-local (check_slot)
FEATURES = ("alts", "yaw", "patch", "meter")
ENABLE = dict(alts=lambda e: e.set_pose_prior(None), yaw=lambda e: e.set_yaw_solve(), patch=lambda e: e.set_patches(),
              meter=lambda e: e.set_metering())
STEP_RECORDS = ("alts", "yaw", "patch")       # what a tiled step and run_post write; ordinary steps: all four


def _stats(e, slot):
    s = capi.FrameStats()
    capi.check(e._L.irmv_engine_frame_stats(e._h, slot, C.byref(s)))
    return bytes(s)


READ = dict(alts=lambda e, s: [bytes(r) for r in e.pose_alts(s)], yaw=lambda e, s: [bytes(r) for r in e.yaw_poses(s)],
            patch=lambda e, s: [bytes(r) for r in e.plate_patches(s)], meter=lambda e, s: [_stats(e, s)])


@contextlib.contextmanager
def group(blob, **kw):
    """{name: engine}: all, all_rev and one engine per feature, each with its features enabled."""
    plan = [("all", FEATURES), ("all_rev", FEATURES[::-1])] + [(f, (f,)) for f in FEATURES]
    with contextlib.ExitStack() as st:
        g = {}
        for name, feats in plan:
            g[name] = st.enter_context(TP.eng(blob, num_slots=SLOTS, **kw))
            for f in feats:
                ENABLE[f](g[name])
        yield g


def compare(g, slots, form, live, seen):
    """Slots' records of every engine of g: results equal everywhere, each side channel of all / all_rev equal to its ONE_x's;
    channels in `live` show a record that is not all zero."""
    for s in slots:
        want = [bytes(d) for d in g["all"].results_raw(s)]
        for name, e in g.items():
            assert [bytes(d) for d in e.results_raw(s)] == want, (form, s, name)
    for f in FEATURES:
        one = [READ[f](g[f], s) for s in slots]
        for name in ("all", "all_rev"):
            assert [READ[f](g[name], s) for s in slots] == one, (form, f, name)
        seen[(form, f)] = sum(any(r) for recs in one for r in recs)
        if f in live:
            assert seen[(form, f)] >= 1, (form, f)


def each(g, fn):
    return [fn(e) for e in g.values()]


def barred(seed):
    """step_frame(seed) with two bright bars 30 px apart, inside the window at CORNERS[1].  They lean by 2 px: the rectangle
    around an upright bar has its sides the other way round and fails the light's ratio gate."""
    img = PS.step_frame(seed).copy()
    _draw_bar(img, (50, 52), (52, 30), 4)
    _draw_bar(img, (80, 52), (82, 30), 4)
    return img


# kind: (environment, engine arguments, the frame of a seed)
KINDS = dict(keypoint=({}, {}, PS.step_frame), device_records=({"IRMV_ZERO_COPY_RESULTS": "0"}, {}, PS.step_frame),
             classical=({}, dict(point_source=capi.POINTS_CLASSICAL, binary_threshold=250), barred))


@pytest.mark.parametrize("kind", list(KINDS))
def test_ordinary_steps_and_run_post(blob, kind, monkeypatch, capsys):
    env, kw, frame = KINDS[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = {}
    with group(blob, **kw) as g:
        a = g["all"]
        each(g, lambda e: TP.put(e, frame(0), True))
        each(g, lambda e: e.detect())
        compare(g, [0], "detect", FEATURES, seen)
        TP.check_slot(a, 0, True)
        for s in range(SLOTS):
            each(g, lambda e: TP.put(e, frame(2 - s), True, s))
        each(g, lambda e: e.submit(0, SLOTS))
        each(g, lambda e: e.wait_slots(0, SLOTS))
        compare(g, range(SLOTS), "submit", FEATURES, seen)
        for s in range(SLOTS):
            TP.check_slot(a, s, True)
        # run_post on the head of slot 0's step (frame 2), while the slot holds frame 0 and that frame's records
        heads = each(g, lambda e: e.read_head(0))
        of_head = [bytes(d) for d in a.results_raw(0)]
        each(g, lambda e: TP.put(e, frame(0), True))
        each(g, lambda e: e.detect())
        assert [bytes(d) for d in a.results_raw(0)] != of_head
        metered = _stats(g["meter"], 0)
        for e, h in zip(g.values(), heads):
            e.write_head(h, 0)
            e.run_post(0, 1)
        compare(g, [0], "run_post", STEP_RECORDS, seen)
        if kind != "classical":      # (a classical engine's records come from the frame as well as from the head)
            assert [bytes(d) for d in a.results_raw(0)] == of_head
        assert _stats(g["meter"], 0) == metered and any(metered)
        TP.check_slot(a, 0, True)
    with capsys.disabled():
        print(f"\n[side records] {kind}: records not all zero {seen}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_tiled_step_and_frame_view(blob, kind, monkeypatch, capsys):
    env, kw, frame = KINDS[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = {}
    img = frame(1)
    with group(blob, window=TP.WIN, **kw) as g:
        a = g["all"]
        for s in range(SLOTS):
            each(g, lambda e: TP.put(e, img, True, s))
        each(g, lambda e: e.submit(0, SLOTS))          # an ordinary step: the slots' metering records
        each(g, lambda e: e.wait_slots(0, SLOTS))
        compare(g, range(SLOTS), "window submit", ("meter",), seen)
        metered = [_stats(g["meter"], s) for s in (1, 2)]
        each(g, lambda e: e.set_tiles(CORNERS, 1))
        each(g, lambda e: e.submit_tiles(0, 1, 2))
        each(g, lambda e: e.wait_slots(1, 2))
        compare(g, [1, 2], "tiled", STEP_RECORDS, seen)
        merged = [bytes(r) for r in a.tile_results_raw(1)[0]]
        assert all([bytes(r) for r in e.tile_results_raw(1)[0]] == merged for e in g.values())
        assert [_stats(g["meter"], s) for s in (1, 2)] == metered
        TP.check_slot(a, 1, True)
        each(g, lambda e: e.set_view("frame"))           # the frame view is built here, behind every enable
        each(g, lambda e: e.detect())
        compare(g, [0], "frame view", FEATURES, seen)
        TP.check_slot(a, 0, True)
    with capsys.disabled():
        print(f"\n[side records] {kind}, window engine: records not all zero {seen}")
