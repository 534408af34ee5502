"""Candidate gather: a step of a sparse-branch engine computes the Detect box branch at the candidate anchors only, one
box_gather launch per level from a compact list (k_boxg.hip), in place of the tile-gated layer launches.  Only the set of
pixels that is computed changes: everything a caller can observe is what an engine created with IRMV_SPARSE_GATHER=0 gives,
bit for bit -- raw tuples, candidate counts, detections, the head read back after the step, the box branch's first convs read
back, a second step after the read-backs, and the cleared bitmap (the runs and the comparison of test_gpu_sparse_branch.py).
The variable is read at engine creation, so every comparison builds separate engines; a dense run is computed once per
configuration and shared.  Engines are created untuned (IRMV_AUTOTUNE=0): no tile choice matters here.

IRMV_SPARSE_GATHER_GRID (a test switch) sets the number of persistent workgroups of a gather launch: with 2 or 3 of them a
workgroup walks several passes of 2 x 16 candidates, which one workgroup per CU never does on these frame counts."""
import functools

import numpy as np
import pytest

import detect_craft as dc
import mem_residue as mr
import test_gpu_lds_residue as lds
import test_gpu_sparse_branch as sb
from irmv_detection_amd import frames
from irmv_detection_amd.engine import YoloEngine

pytestmark = pytest.mark.gpu

NC = 14
PASS = 32                # candidates of a workgroup's pass: two groups of 16 (k_boxg.hip GNG)
SMALL_GRID = 2
_dense = {}


def _pair(blob, monkeypatch, imgs, slots, thr, net, streams, key, grid=None, net_height=None):
    """-> (the IRMV_SPARSE_GATHER=0 engine's run, the gather engine's run): test_gpu_sparse_branch._run's records and plans."""
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    if net_height is not None:
        monkeypatch.setattr(sb, "YoloEngine", functools.partial(YoloEngine, net_height=net_height))
    k = (key, slots, thr, net, net_height, streams, len(imgs))
    if k not in _dense:
        monkeypatch.setenv("IRMV_SPARSE_GATHER", "0")
        monkeypatch.delenv("IRMV_SPARSE_GATHER_GRID", raising=False)
        _dense[k] = sb._run(blob, monkeypatch, imgs, True, slots, thr, net=net, streams=streams)
    monkeypatch.delenv("IRMV_SPARSE_GATHER", raising=False)
    if grid is None:
        monkeypatch.delenv("IRMV_SPARSE_GATHER_GRID", raising=False)
    else:
        monkeypatch.setenv("IRMV_SPARSE_GATHER_GRID", str(grid))
    return _dense[k], sb._run(blob, monkeypatch, imgs, True, slots, thr, net=net, streams=streams)


def _gather_plan(plan):
    """The step of a gathering engine: box_gather_* for all three levels behind the last class carrier, no layer launch of
    the box branch."""
    layers = [l for l, _ in plan]
    names = dict(plan)
    last_cls = max(i for i, l in enumerate(layers) if l.startswith("model.22.cv3.") and l.endswith(".1"))
    for lv, cin in enumerate((64, 128, 256)):
        g = f"model.22.cv2.{lv}.g"
        assert g in layers and layers.index(g) > last_cls and names[g] == f"box_gather_c{cin}", plan
        assert f"model.22.cv2.{lv}.0" not in layers and f"model.22.cv2.{lv}.1" not in layers, layers


def _layer_plan(plan):
    """Today's step: the box branch as layer launches, no gather."""
    layers = [l for l, _ in plan]
    assert not any(l.endswith(".g") for l in layers) and not any(n.startswith("box_gather") for _, n in plan), plan
    assert any(l.startswith(("model.22.cv2.0.1", "model.22.cv2.0.0", "model.22.s0.0")) for l in layers), layers


def _lit_bias():
    b = np.full(NC, dc.DARK, np.float32)
    b[3] = 2.0           # sigmoid 0.88: a candidate at 0.25 at every anchor of the level
    return b


@pytest.mark.parametrize("lit", [(0,), (1,), (2,), (0, 1, 2)])
@pytest.mark.parametrize("net,net_height", [(64, None), (96, 64)])
def test_every_anchor_a_candidate_on_the_smallest_maps(blob, monkeypatch, net, net_height, lit):
    """Class finals crafted to a constant bias light whole levels (every anchor of a lit level a candidate, none on the
    others) while the box weights stay real.  Net 64 x 64: 8 x 8 / 4 x 4 / 2 x 2 maps -- on the last one every neighbourhood
    leaves the map on two sides; 96 x 64: 12 x 8 / 6 x 4 / 3 x 2.  Three slots on one stream share, two workgroups: borders,
    corners, overlapping neighbourhoods, lists of 192 / 48 / 12 and 288 / 72 / 18 candidates -- several passes per workgroup,
    lengths that are no multiple of 16 -- and empty lists beside them."""
    cls = {lv: ("bias", _lit_bias() if lv in lit else dc.dark_bias(NC)) for lv in range(3)}
    crafted = dc.craft(blob, cls=cls)
    imgs = [frames.synthetic_frame(i) for i in range(6)]
    want, got = _pair(crafted, monkeypatch, imgs, 3, 0.25, net, 1, ("lit", lit), grid=SMALL_GRID, net_height=net_height)
    sb._compare(want[0], got[0])
    _gather_plan(got[1])
    _layer_plan(want[1])
    H, W = (net_height or net), net
    hw = [(H // s) * (W // s) for s in (8, 16, 32)]
    lt = sb._logit_thr(0.25)
    for rec in want[0]:                      # by the dense head: exactly the lit levels' anchors are candidates
        cand = (rec[3][:, 64:64 + NC] > lt).any(1)
        base = 0
        for lv in range(3):
            assert cand[base:base + hw[lv]].all() if lv in lit else not cand[base:base + hw[lv]].any(), (lv, lit)
            base += hw[lv]
    assert 3 * hw[0] > SMALL_GRID * PASS or 0 not in lit


REAL = [(640, 8, 0.25, None), (640, 8, sb.HIGH_THR, None), (640, 3, 0.25, SMALL_GRID), (640, 3, sb.HIGH_THR, SMALL_GRID),
        (320, 8, 0.25, None), (320, 3, sb.HIGH_THR, SMALL_GRID)]


@pytest.mark.parametrize("net,slots,thr,grid", REAL)
def test_real_frames(blob, rm_test_image, monkeypatch, net, slots, thr, grid):
    """Frames 0 .. 15, 100 and rm_test.jpg on two streams (shares of four images, and of two and one), at score_thr 0.25 and at
    0.9, which leaves isolated candidates: images without a candidate beside images with some, short unequal lists; the
    three-slot engines with two workgroups per launch."""
    imgs = sb._images(rm_test_image)
    want, got = _pair(blob, monkeypatch, imgs, slots, thr, net, 2, "real", grid=grid)
    sb._compare(want[0], got[0])
    _gather_plan(got[1])
    _layer_plan(want[1])
    with_cand = sum(w[1] > 0 for w in want[0])
    if net == 640:       # (the counts test_gpu_sparse_branch.py asserts for this frame set)
        assert with_cand >= (14 if thr == 0.25 else 10)
    assert 2 <= with_cand < len(imgs)       # lists with entries in more than one launch, and frame 100's empty ones


def test_the_frame_sets_reach_the_gathers_edges(blob, rm_test_image, monkeypatch):
    """Nothing vacuous, from the dense engines' heads.  Over both frame sets, on every level candidates in the first and the
    last row and column: the 1280 x 1024 frames are letterboxed, so the first and last rows of their maps hold no candidate and
    the lit 64 x 64 set is what reaches those (its maps counted here next to the real ones').  On the real frames: two
    candidates that are 8-neighbours (their neighbourhoods overlap); a level of a frame with exactly one candidate; a launch
    whose list is longer than its workgroups' first pass; an image without a candidate beside one that has some."""
    imgs = sb._images(rm_test_image)
    maps = []
    for thr in (0.25, sb.HIGH_THR):
        want, _ = _pair(blob, monkeypatch, imgs, 3, thr, 640, 2, "real", grid=SMALL_GRID)
        maps.append(sb._cand_maps(want[0], thr, 640))
    lit = dc.craft(blob, cls={lv: ("bias", _lit_bias()) for lv in range(3)})
    want, _ = _pair(lit, monkeypatch, [frames.synthetic_frame(i) for i in range(6)], 3, 0.25, 64, 1, ("lit", (0, 1, 2)), grid=SMALL_GRID)
    small = sb._cand_maps(want[0], 0.25, 64)
    for lv in range(3):
        edges = [False] * 4
        for f in maps[0] + small:
            m = f[lv]
            edges = [e or bool(x) for e, x in zip(edges, (m[0].any(), m[-1].any(), m[:, 0].any(), m[:, -1].any()))]
        assert all(edges), (lv, edges)
    nb = False
    for f in maps[0]:
        for m in f:
            nb = nb or (m[:, 1:] & m[:, :-1]).any() or (m[1:] & m[:-1]).any() or (m[1:, 1:] & m[:-1, :-1]).any() or (m[1:, :-1] & m[:-1, 1:]).any()
    assert nb
    assert any(int(m.sum()) == 1 for f in maps[1] for m in f)
    # the three-slot engine on two streams launches images (0, 1) and (2) of every round of three
    longest = max(int(maps[0][f][0].sum() + (maps[0][f + 1][0].sum() if f + 1 < len(imgs) else 0)) for f in range(0, len(imgs), 3))
    assert longest > SMALL_GRID * PASS, longest
    beside = [False] * 3
    for f in range(0, len(imgs) - 1, 3):
        for lv in range(3):
            beside[lv] = beside[lv] or (maps[1][f][lv].any() != maps[1][f + 1][lv].any())
    assert all(beside), beside


def _plan_of(blob, slots, **kw):
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=slots, **kw) as e:
        e.get_src_image_buffer(0)[:] = frames.synthetic_frame(1)
        return [(st["layer"], st["name"]) for st in e.profile(0, slots)]


def test_plan(blob, monkeypatch):
    """The default batched engine gathers; IRMV_SPARSE_GATHER=0, IRMV_FORCE_WRES and a single-slot engine launch today's lists."""
    for v in ("IRMV_SPARSE_GATHER", "IRMV_SPARSE_GATHER_GRID", "IRMV_FORCE_WRES", "IRMV_SPARSE_BRANCH", "IRMV_SPARSE_HEAD", "IRMV_AUTOTUNE"):
        monkeypatch.delenv(v, raising=False)
    _gather_plan(_plan_of(blob, 4, num_streams=2))
    monkeypatch.setenv("IRMV_SPARSE_GATHER", "0")
    off = _plan_of(blob, 4, num_streams=2)
    _layer_plan(off)
    sb._gated_plan(off, [])
    monkeypatch.delenv("IRMV_SPARSE_GATHER")
    monkeypatch.setenv("IRMV_FORCE_WRES", "3")
    wres = _plan_of(blob, 4, num_streams=2)
    _layer_plan(wres)
    sb._gated_plan(wres, ["model.22.cv2.0.0"])
    monkeypatch.delenv("IRMV_FORCE_WRES")
    _layer_plan(_plan_of(blob, 1))


def test_rows_as_the_step_left_them(blob, monkeypatch):
    """test_gpu_sparse_branch's sentinel test on the gather engine (its `branch` engine is the default one): candidate rows
    are the dense rows, every other row and every class channel is still the sentinel."""
    monkeypatch.delenv("IRMV_SPARSE_GATHER", raising=False)
    monkeypatch.delenv("IRMV_SPARSE_GATHER_GRID", raising=False)
    monkeypatch.delenv("IRMV_AUTOTUNE", raising=False)
    _gather_plan(_plan_of(blob, 8))
    sb.test_rows_as_the_step_left_them(blob, monkeypatch)


def test_no_output_depends_on_lds_or_device_memory_residue(blob, monkeypatch):
    """A three-slot 320 engine whose profile shows the gather launches: the batched step and detect() under the three LDS
    fills (test_gpu_lds_residue._residue_run), then the batched step under every device-memory fill (mem_residue.PATTERNS:
    the candidate lists are scratch, filled with in-range garbage) against the unfilled step."""
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.delenv("IRMV_SPARSE_GATHER", raising=False)
    monkeypatch.delenv("IRMV_SPARSE_GATHER_GRID", raising=False)
    make = lambda: YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=3, net_size=320, num_streams=1)   # noqa: E731
    imgs = [frames.synthetic_frame(3 + i) for i in range(3)]
    differ, names, _, _ = lds._residue_run(make, 3, imgs)
    assert {"box_gather_c64", "box_gather_c128", "box_gather_c256"} <= names, names
    assert not differ, differ[:20]
    with make() as e:
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
