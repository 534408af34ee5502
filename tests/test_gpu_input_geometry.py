"""The input stage on the whole zoo of tests/input_geometry.py: every entry as two engines -- the default plan, and
IRMV_FUSED_FRONT = IRMV_FUSED_C2F = IRMV_FUSED_HEAD = 0 -- with launch choices pinned untimed, a distinct frame in every slot.

Per entry:
  * the profile lists front_fused exactly when irmv_front_plan says fused;
  * read_input of both engines, on every slot, is bitwise the oracle's preprocess of that slot's frame rounded to fp16
    (a Bayer entry's frame is bayer.demosaic of its raw frame; on a rectangular net the oracle's numpy restatement
    tests/rect_ref.py, which tests/test_input_geometry.py holds bitwise to the oracle on every square entry);
  * get_rotated_image(slot) is frame[::-1, ::-1] on every slot -- for Bayer entries the demosaic's bit-exact check at
    misaligned slot bases;
  * taps "0" and "1" are bitwise equal between the two engines on every slot;
  * on the unfused engine tap "0" is within bound() (tests/test_gpu_conv_candidates.py) of tests/conv_ref.py on the engine's
    own "input", tap "1" within bound() of conv_ref on the engine's own tap "0", and channel 3 of "input" is +0 everywhere;
  * every launch form gives the same bits (frames moved one slot on between forms, so a stale tensor cannot pass):
    detect(slot) per slot, the batched step over all slots, and a stream share submitted alone.  A 3-slot engine takes
    as many streams as slots by default and would cut every step into single frames, so the stream count is set: the
    default-plan engine has ONE stream -- the batched step is one launch of 3 frames behind one copy-engine upload of 3
    frames (detect() uploads a frame with the upload kernel where its slot is aligned), followed by slots 1 .. 2 as a
    step of 2 frames from a slot base that is not the engine's first -- and the unfused engine has TWO: the batched
    step is a share of 2 frames beside one of 1, and slots 0 .. 1 submitted alone are the first stream's share.  So the
    front kernel's tile-to-frame mapping runs at batch 3 and 2, the demosaic at batch 3 and 2, preprocess at batch 2.

Parametrised by group of categories, not by entry.  No entry is skipped."""
import time

import numpy as np
import pytest

import conv_ref
import input_geometry as ig
import rect_ref
from irmv_detection_amd import capi
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_gpu_conv_candidates import bound, layer_table, read

pytestmark = pytest.mark.gpu

TAPS = ("input", "0", "1")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_input(hwc, e):
    W, H = e.net
    x = oracle.preprocess(hwc, W, e.mode, e.rot, e.swap) if W == H else rect_ref.preprocess(hwc, W, H, e.mode, e.rot, e.swap)
    return x.astype(np.float16).astype(np.float32)


def snapshot(eng, slot):
    return {t: (eng.read_input(slot) if t == "input" else eng.read_tap(t, slot)).copy() for t in TAPS}


def same(a, b):
    return [t for t in TAPS if not np.array_equal(bits(a[t]), bits(b[t]))]


def check_entry(e, blob, table, monkeypatch):
    W, H = e.net
    S = e.slots
    fr = ig.slot_frames(e)
    plan = capi.front_plan(e.src, W, H, e.mode, e.rot, capi.SRC_HWC8 if e.fmt == "HWC" else e.fmt)
    assert plan["fused"] == (e.expect == ig.FUSED), (e.name, plan)
    want = [oracle_input(hwc, e) for _, hwc in fr]
    kw = dict(weights_blob=blob, net_size=W, net_height=H, resize_mode=e.mode, rotate180=e.rot, swap_rb=e.swap, num_slots=S,
              src_format=capi.SRC_HWC8 if e.fmt == "HWC" else e.fmt, bayer_gains=e.gains)
    snaps = {}
    for fused in (True, False):
        for k in ("IRMV_FUSED_FRONT", "IRMV_FUSED_C2F", "IRMV_FUSED_HEAD"):
            if fused:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, "0")
        with YoloEngine(None, e.src, num_streams=1 if fused else min(S, 2), **kw) as eng:
            share = -(-S // eng.num_streams)
            assert share == ((3 if fused else 2) if S == 3 else 1), (e.name, S, eng.num_streams)
            names = [k["name"] for k in eng.profile(0, 1)]
            assert ("front_fused" in names) == (fused and plan["fused"]), (e.name, fused, names[:4])
            assert ("bayer_demosaic" in names) == (e.fmt != "HWC"), (e.name, names[:4])
            # form 1: one synchronous detect() per slot
            for s in range(S):
                eng.get_src_image_buffer(s)[:] = fr[s][0]
            snap = []
            for s in range(S):
                eng.detect(s)
                snap.append(snapshot(eng, s))
                assert np.array_equal(bits(snap[s]["input"]), bits(want[s])), (e.name, fused, s, "input differs from the oracle",
                                                                              float(np.abs(snap[s]["input"] - want[s]).max()))
                assert np.array_equal(eng.get_rotated_image(s), fr[s][1][::-1, ::-1]), (e.name, fused, s, "rotated image")
            snaps[fused] = snap
            # form 2: the batched step over all slots, every frame one slot on
            for s in range(S):
                eng.get_src_image_buffer((s + 1) % S)[:] = fr[s][0]
            eng.submit(0, S)
            eng.wait()
            for s in range(S):
                assert not same(snapshot(eng, (s + 1) % S), snap[s]), (e.name, fused, "batched", s)
                assert np.array_equal(eng.get_rotated_image((s + 1) % S), fr[s][1][::-1, ::-1]), (e.name, fused, "batched", s)
            # form 3: a part of the engine alone, its frames moved on once more: slots 1 .. 2 of the one-stream engine, the
            # first stream's share (slots 0 .. 1) of the two-stream engine; the one slot of a 1-slot engine
            first, count = (0, 1) if S == 1 else ((1, 2) if fused else (0, share))
            for s in range(first, first + count):
                eng.get_src_image_buffer(s)[:] = fr[(s + 2) % S][0]
            eng.submit(first, count)
            eng.wait()
            for s in range(first, first + count):
                assert not same(snapshot(eng, s), snap[(s + 2) % S]), (e.name, fused, "part", s)
                assert np.array_equal(eng.get_rotated_image(s), fr[(s + 2) % S][1][::-1, ::-1]), (e.name, fused, "part", s)
            if not fused:   # the layers against their references, on the engine's own tensors (every slot holds some frame of the entry)
                (w0, b0), (w1, b1) = table["model.0.conv"], table["model.1.conv"]
                for s in range(S):
                    x_raw = read(eng, "input", s, 1)[0]
                    assert x_raw.shape == (H, W, 4) and (x_raw[..., 3] == 0).all(), (e.name, s, "channel 3 of input is not +0 everywhere")
                    t0 = conv_ref.decode(read(eng, "0", s, 1)[0], "0")
                    t1 = conv_ref.decode(read(eng, "1", s, 1)[0], "1")
                    y0, a0 = conv_ref.conv0(conv_ref.decode(x_raw, "input"), w0, b0)
                    r0 = float((np.abs(t0 - y0) / bound(y0, a0, False)).max())
                    y1, a1 = conv_ref.conv(t0, w1, b1, 2, 1)
                    r1 = float((np.abs(t1 - y1) / bound(y1, a1, False)).max())
                    assert r0 <= 1.0 and r1 <= 1.0, (e.name, s, r0, r1)
    for s in range(S):
        differ = [t for t in ("0", "1") if not np.array_equal(bits(snaps[True][s][t]), bits(snaps[False][s][t]))]
        assert not differ, (e.name, s, differ, plan)
    return plan


@pytest.mark.parametrize("group", ig.GROUPS)
def test_input_stage_on_the_zoo(blob, monkeypatch, capsys, group):
    # both engines take the untimed launch choices (as test_profile_lists_the_demosaic_only_for_bayer_engines pins them):
    # what is compared is bits and the step's shape, and creation stays short
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_FORCE", "1")
    table = layer_table(blob)
    entries = [e for e in ig.ZOO if ig.group_of(e) == group]
    assert entries
    t0 = time.time()
    fused = 0
    for e in entries:
        fused += check_entry(e, blob, table, monkeypatch)["fused"]
    with capsys.disabled():
        print(f"\n[input zoo: {group}] {len(entries)} entries ({fused} fused), {sum(e.slots for e in entries)} frames, {time.time() - t0:.1f} s")
