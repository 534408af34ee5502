"""Candidate gather, keypoint branch: a level's box_gather launch computes the level's keypoint branch too (a fourth wave per
group, k_boxg.hip) and the step drops the tile-gated kpt3_* launch.  Only the launch that computes the rows changes: everything
a caller can observe is what an engine created with IRMV_GATHER_KPT=0 gives, bit for bit -- raw tuples, candidate counts,
detections, the head read back, the box branch's first convs and the keypoint branch's 22.cv4.L.{0,1} read back, a second step
after the read-backs, and the cleared bitmap (the runs and the comparison of test_gpu_sparse_branch.py, with the keypoint
tensors added to its read-backs).  The variable is read at engine creation, so every comparison builds separate engines; an
IRMV_GATHER_KPT=0 run is computed once per configuration and shared.  Engines are created untuned (IRMV_AUTOTUNE=0)."""
import functools

import numpy as np
import pytest

import detect_craft as dc
import mem_residue as mr
import test_gpu_lds_residue as lds
import test_gpu_sparse_branch as sb
import test_gpu_sparse_gather as sg
from irmv_detection_amd import frames, weights
from irmv_detection_amd.engine import YoloEngine
from test_gpu_engine import _load, _raw_tuple

pytestmark = pytest.mark.gpu

NC, NK = 14, 8
KPT_COLS = slice(64 + NC, 64 + NC + NK)
TAPS = sb.TAPS + tuple(f"22.cv4.{lv}.{k}" for lv in range(3) for k in (0, 1))
SWITCHES = ("IRMV_GATHER_KPT", "IRMV_KPT3", "IRMV_SPARSE_GATHER", "IRMV_SPARSE_GATHER_GRID", "IRMV_FORCE_WRES", "IRMV_SPARSE_BRANCH", "IRMV_SPARSE_HEAD")
_off = {}


def _clean(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")


def _pair(blob, monkeypatch, imgs, slots, thr, net, streams, key, grid=None, net_height=None):
    """-> (the IRMV_GATHER_KPT=0 engine's run, the default engine's run): test_gpu_sparse_branch._run's records and plans."""
    _clean(monkeypatch)
    monkeypatch.setattr(sb, "TAPS", TAPS)
    if net_height is not None:
        monkeypatch.setattr(sb, "YoloEngine", functools.partial(YoloEngine, net_height=net_height))
    if grid is not None:
        monkeypatch.setenv("IRMV_SPARSE_GATHER_GRID", str(grid))
    k = (key, slots, thr, net, net_height, streams, grid, len(imgs))
    if k not in _off:
        monkeypatch.setenv("IRMV_GATHER_KPT", "0")
        _off[k] = sb._run(blob, monkeypatch, imgs, True, slots, thr, net=net, streams=streams)
        monkeypatch.delenv("IRMV_GATHER_KPT")
    return _off[k], sb._run(blob, monkeypatch, imgs, True, slots, thr, net=net, streams=streams)


def _kpt_names(plan):
    return sorted(n for _, n in plan if n.startswith("kpt3_"))


def _fused_plan(plan):
    """The gathers behind the last class carrier, and the keypoint branch neither as kpt3_* launches nor as layers."""
    sg._gather_plan(plan)
    assert not _kpt_names(plan) and not any(l.startswith("model.22.cv4.") for l, _ in plan), plan


def _parent_plan(plan):
    """The three gathers AND the three kpt3_* launches."""
    sg._gather_plan(plan)
    assert _kpt_names(plan) == ["kpt3_c128", "kpt3_c256", "kpt3_c64"], plan


def test_plan(blob, monkeypatch):
    _clean(monkeypatch)
    _fused_plan(sg._plan_of(blob, 4, num_streams=2))
    monkeypatch.setenv("IRMV_GATHER_KPT", "0")
    off = sg._plan_of(blob, 4, num_streams=2)
    _parent_plan(off)
    single = sg._plan_of(blob, 1)
    monkeypatch.delenv("IRMV_GATHER_KPT")
    monkeypatch.setenv("IRMV_KPT3", "1")
    named = sg._plan_of(blob, 4, num_streams=2)
    _parent_plan(named)
    assert named == off
    monkeypatch.delenv("IRMV_KPT3")
    monkeypatch.setenv("IRMV_SPARSE_GATHER", "0")
    layers = sg._plan_of(blob, 4, num_streams=2)
    sg._layer_plan(layers)
    assert _kpt_names(layers) == ["kpt3_c128", "kpt3_c256", "kpt3_c64"], layers
    monkeypatch.delenv("IRMV_SPARSE_GATHER")
    one = sg._plan_of(blob, 1)
    sg._layer_plan(one)
    assert one == single        # a single-frame plan does not gather: the switch changes nothing


@pytest.mark.parametrize("lit", [(0,), (1,), (2,), (0, 1, 2)])
@pytest.mark.parametrize("net,net_height", [(64, None), (96, 64)])
def test_every_anchor_a_candidate_on_the_smallest_maps(blob, monkeypatch, net, net_height, lit):
    """test_gpu_sparse_gather's lit maps (8 x 8 / 4 x 4 / 2 x 2 and 12 x 8 / 6 x 4 / 3 x 2, three slots, two workgroups):
    borders and corners on every side, several passes per workgroup, list lengths off 16, empty lists beside full ones.  The
    keypoint weights stay real."""
    cls = {lv: ("bias", sg._lit_bias() if lv in lit else dc.dark_bias(NC)) for lv in range(3)}
    crafted = dc.craft(blob, cls=cls)
    imgs = [frames.synthetic_frame(i) for i in range(6)]
    want, got = _pair(crafted, monkeypatch, imgs, 3, 0.25, net, 1, ("lit", lit), grid=sg.SMALL_GRID, net_height=net_height)
    sb._compare(want[0], got[0])
    _fused_plan(got[1])
    _parent_plan(want[1])
    H, W = (net_height or net), net
    hw = [(H // s) * (W // s) for s in (8, 16, 32)]
    for rec in want[0]:                      # not vacuous: the keypoint columns of the lit levels' rows hold values
        base = 0
        for lv in range(3):
            if lv in lit:
                assert (rec[3][base:base + hw[lv], KPT_COLS] != 0).any(1).all(), (lv, lit)
            base += hw[lv]


REAL = [(640, 8, 0.25, 2, None), (640, 8, sb.HIGH_THR, 2, None), (640, 3, 0.25, 2, sg.SMALL_GRID), (640, 3, sb.HIGH_THR, 2, sg.SMALL_GRID),
        (416, 3, 0.25, 2, None)]


@pytest.mark.parametrize("net,slots,thr,streams,grid", REAL)
def test_real_frames(blob, rm_test_image, monkeypatch, net, slots, thr, streams, grid):
    """Frames 0 .. 15, 100 and rm_test.jpg: net 640 with 8 slots on two streams and with 3 slots and two workgroups, at 0.25
    and at 0.9 (isolated candidates, images without one); net 416 (52 / 26 / 13 maps: no multiple of anything) with 3 slots."""
    imgs = sb._images(rm_test_image)
    want, got = _pair(blob, monkeypatch, imgs, slots, thr, net, streams, "real", grid=grid)
    sb._compare(want[0], got[0])
    _fused_plan(got[1])
    _parent_plan(want[1])
    lt = sb._logit_thr(thr)
    cand = [(w[3][:, 64:64 + NC] > lt).any(1) for w in want[0]]
    assert sum(int(c.sum()) for c in cand) > 0
    assert any((w[3][c][:, KPT_COLS] != 0).any() for w, c in zip(want[0], cand))


def test_rows_as_the_step_left_them(blob, monkeypatch):
    """A decoy in every head row, a step, then the head as it lies in memory (debug_read_head_raw): at the candidate anchors
    the box and keypoint columns are the dense head's, every other row and every class column is still the decoy -- and the
    whole storage is what the IRMV_GATHER_KPT=0 engine leaves."""
    _clean(monkeypatch)
    imgs = [frames.synthetic_frame(8 + i) for i in range(8)]
    lt = sb._logit_thr(0.25)
    raws = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("IRMV_GATHER_KPT")
        else:
            monkeypatch.setenv("IRMV_GATHER_KPT", mode)
        with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=8) as e:
            plan = [(st["layer"], st["name"]) for st in e.profile(0, 8)]
            (_parent_plan if mode == "0" else _fused_plan)(plan)
            decoy = [dc.decoy_head(e.num_anchors, e.head_channels, NC, 77 + s) for s in range(8)]
            for s in range(8):
                e.write_head(decoy[s], s)
                _load(e, s, imgs[s])
            e.submit(0, 8); e.wait()
            raw = [e.debug_read_head_raw(s).copy() for s in range(8)]
            dense = [e.read_head(s).copy() for s in range(8)]
        raws[mode] = raw
        total = 0
        for s in range(8):
            cand = (dense[s][:, 64:64 + NC] > lt).any(1)
            total += int(cand.sum())
            for c in (slice(0, 64), KPT_COLS):
                assert np.array_equal(raw[s][cand][:, c], dense[s][cand][:, c]), (mode, s, c)
            assert np.array_equal(raw[s][~cand], decoy[s][~cand]), (mode, s, np.nonzero((raw[s] != decoy[s]).any(1) & ~cand)[0][:8])
            assert np.array_equal(raw[s][:, 64:64 + NC], decoy[s][:, 64:64 + NC]), (mode, s)
        assert total > 400
    for s in range(8):
        assert np.array_equal(raws["0"][s], raws[None][s]), s


def test_no_output_depends_on_lds_or_device_memory_residue(blob, monkeypatch):
    """The three-slot 320 engine of test_gpu_sparse_gather's residue test, its gathers now with the keypoint wave and its
    planes: the batched step and detect() under the three LDS fills, then the batched step under every device-memory fill."""
    _clean(monkeypatch)
    make = lambda: YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=3, net_size=320, num_streams=1)   # noqa: E731
    imgs = [frames.synthetic_frame(3 + i) for i in range(3)]
    differ, names, _, _ = lds._residue_run(make, 3, imgs)
    assert {"box_gather_c64", "box_gather_c128", "box_gather_c256"} <= names, names
    assert not differ, differ[:20]
    with make() as e:
        plan = [(st["layer"], st["name"]) for st in e.profile(0, 3)]
        _fused_plan(plan)
        for s in range(3):
            e.get_src_image_buffer(s)[:] = imgs[s]
        taps = lds._tensors(e)
        e.submit(0, 3); e.wait()
        ref = lds._snapshot(e, [0, 1, 2], [0, 2], taps, None)
        assert sum(e.read_raw(s)["n_candidates"] for s in range(3)) > 0
        for p in mr.PATTERNS:
            e.debug_fill_mem(p)
            e.submit(0, 3); e.wait()
            snap = lds._snapshot(e, [0, 1, 2], [0, 2], taps, None)
            assert [k for k, v in ref.items() if snap[k] != v] == [], hex(p)
            assert not mr.carried_nonzero(e)


def test_a_model_without_a_keypoint_head_keeps_the_box_only_gather(monkeypatch):
    """nk = 0: no OP_KPT3 op to link, the gather runs its box-only form -- the plan and every bit are the IRMV_GATHER_KPT=0
    engine's.  (The engine accepts nk = 0 and nk = 8 only: there is no other head shape to run.)"""
    _clean(monkeypatch)
    blob0 = weights.synthetic_blob(nk=0)
    imgs = [frames.synthetic_frame(i) for i in range(3)]
    runs = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("IRMV_GATHER_KPT")
        else:
            monkeypatch.setenv("IRMV_GATHER_KPT", mode)
        with YoloEngine(None, (1280, 1024), weights_blob=blob0, num_slots=3, net_size=320, num_streams=1) as e:
            for s in range(3):
                _load(e, s, imgs[s])
            e.submit(0, 3); e.wait()
            raws = [_raw_tuple(e.read_raw(s)) for s in range(3)]
            ncand = [e.read_raw(s)["n_candidates"] for s in range(3)]
            heads = [e.read_head(s).copy() for s in range(3)]
            plan = [(st["layer"], st["name"]) for st in e.profile(0, 3)]
        assert not _kpt_names(plan) and sum(n.startswith("box_gather_c") for _, n in plan) == 3, plan
        runs[mode] = (raws, ncand, heads, plan)
    a, b = runs["0"], runs[None]
    assert a[3] == b[3]
    assert a[1] == b[1]
    assert all(sb._same_raw(x, y) for x, y in zip(a[0], b[0]))
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
