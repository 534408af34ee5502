"""Tiled search on the GPU: N window slots run their windows of ONE frame in one step, and the step's last node merges their
result lists (irmv_engine_submit_tiles; k_tiles.hip).

Two claims, no tolerance anywhere:
  * behind the crop every tile is the window engine -- its snapshot (input, head, raw, dets, pose) equals
    test_gpu_window.reference at its corner, the plain engine on the host crop;
  * the merged list is irmv_detection_amd.tiles.merge of the per-slot results: the same (tile, index, cut) list, and records
    byte-identical to irmv_engine_results.

The blobs are test_gpu_window's (class biases shifted up, an armor-like keypoint quad), so the frames hold detections with
solved poses; the crafted cases write heads built here -- chosen anchors, hot DFL bins -- and run decode + NMS + merge alone.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import detect_craft as dc
import tile_ladder as tl
from irmv_detection_amd import bayer, capi, tiles
from test_gpu_window import FULL, WIN, _hip_memcpy_h2d, frame_of, peng, reference, same_results, same_tensors, snapshot, weng

pytestmark = pytest.mark.gpu

CORNERS4 = [(0, 0), (66, 0), (0, 73), (66, 73)]            # the four extreme windows of the 322 x 201 frame
FULL2, WIN2 = (320, 200), (128, 64)                       # 3 x 4 grid at overlap (32, 16); the net is the window, 1 : 1
MERGE_FRAME = 21                                          # synthetic frame whose 3 x 4 tiles see armors twice (asserted below)


@pytest.fixture(scope="module")
def wblob(blob):
    return dc.craft(blob, cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))


def slot_lists(e, first, count):
    """Per tile: the slot's irmv_engine_results as the merge reference takes them, and the records' bytes."""
    lists, raw = [], []
    for s in range(first, first + count):
        n = C.c_int(0)
        buf = (capi.Det * e.max_det)()
        capi.check(e._L.irmv_engine_results(e._h, s, buf, e.max_det, C.byref(n)))
        lists.append(dict(boxes=np.array([list(buf[i].xyxy) for i in range(n.value)], np.float32).reshape(-1, 4),
                          scores=np.array([buf[i].score for i in range(n.value)], np.float32),
                          classes=np.array([buf[i].class_id for i in range(n.value)], int)))
        raw.append([bytes(buf[i]) for i in range(n.value)])
    return lists, raw


def check_merge(e, first, corners, frame_size, win, ios_thr=tiles.DEFAULT_IOS_THR, edge_margin=tiles.DEFAULT_EDGE_MARGIN):
    """tile_results(first) against tiles.merge of the slots' results; returns the reference's trace."""
    recs, n_in = e.tile_results_raw(first)
    lists, raw = slot_lists(e, first, len(corners))
    kept, trace = tiles.merge(lists, corners, win, frame_size, ios_thr, edge_margin, e.max_det)
    assert n_in == sum(len(r) for r in raw) == len(trace)
    assert [(r.tile, r.index, r.cut) for r in recs] == kept
    for r in recs:
        assert bytes(r.det) == raw[r.tile][r.index] and r.reserved == 0
    return trace


def cross_tile_suppressions(trace):
    return sum(t["rule"] == "suppressed" for t in trace)


# ---- 1. each tile is the window engine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False])
def test_each_tile_is_the_window_engine(wblob, rot):
    frame = frame_of(12)
    others = [frame_of(60 + s) for s in range(5)]
    solved = 0
    with weng(wblob, num_slots=5, rotate180=rot) as w:
        g0 = w.debug_graph_count()
        for frame_slot in (0, 2):                       # outside and inside the tiles' range [1, 5)
            for s in range(5):
                w.get_src_image_buffer(s)[:] = frame if s == frame_slot else others[s]
            w.set_tiles(CORNERS4, first=1)
            w.submit_tiles(frame_slot, 1, 4)
            w.wait_slots(1, 4)
            for t, org in enumerate(CORNERS4):
                got, ref = snapshot(w, 1 + t), reference(wblob, frame, org, rot, tag="f12")
                same_tensors(got, ref)
                solved += same_results(got, ref, org, (frame_slot, t))
            check_merge(w, 1, CORNERS4, FULL, WIN)
            for s in range(5):                          # no pinned slot was written
                assert np.array_equal(w.get_src_image_buffer(s), frame if s == frame_slot else others[s])
        assert w.debug_graph_count() == g0 + 2          # one graph per frame_slot
    assert solved > 0


# ---- 2. the merged list is the host reference's -----------------------------------------------------------------------------------
def test_merged_list_matches_the_host_reference(wblob):
    corners, nx, ny = capi.tile_grid(FULL2, WIN2, (32, 16), net_size=WIN2[0], net_height=WIN2[1])
    assert (nx, ny) == (3, 4)
    with weng(wblob, full=FULL2, win=WIN2, net=WIN2, num_slots=13) as w:
        assert w.tile_grid((32, 16)) == (corners, 3, 4)
        assert w.tile_merge == (0.5, 2.0)
        w.get_src_image_buffer(0)[:] = frame_of(MERGE_FRAME, FULL2)
        w.set_tiles(corners, first=1)
        w.submit_tiles(0, 1, 12)
        w.wait_slots(1, 12)
        trace = check_merge(w, 1, corners, FULL2, WIN2)
        assert cross_tile_suppressions(trace) >= 1
        assert sum(t["rule"] == "kept" for t in trace) >= 2
        merged = w.tile_results(1)
        assert len(merged) == sum(t["rule"] == "kept" for t in trace) and any(a.pnp_ok for a in merged)


# ---- 3. crafted results ----------------------------------------------------------------------------------------------------------
def crafted_head(e, net, recs):
    """A head with the given detections and nothing else.  recs: (level, ix, iy, (l, t, r, b), cls, logit); a side is a
    number of strides in halves: k puts all DFL mass on bin k, k + 0.5 half on k and half on k + 1.  The box is
    ((ix + .5 - l) s, (iy + .5 - t) s, (ix + .5 + r) s, (iy + .5 + b) s) in net-input pixels."""
    A, no = e.num_anchors, e.head_channels
    nc = no - 64 - 8
    h = np.zeros((A, no), np.float32)
    h[:, :64] = dc.dfl_bias(0)
    h[:, 64:64 + nc] = dc.DARK
    h[:, 64 + nc:] = dc.quad_kpt_bias(8)
    bases = dc.level_bases(net[0], net[1])
    for level, ix, iy, sides, cls, logit in recs:
        a = bases[level] + iy * (net[0] // dc.STRIDES[level]) + ix
        for j, d in enumerate(sides):
            h[a, 16 * j:16 * j + 16] = dc.OFF_BIN
            h[a, 16 * j + int(d)] = 0.0
            if d != int(d):
                h[a, 16 * j + int(d) + 1] = 0.0
        h[a, 64 + cls] = np.float32(logit)
    return h


# three tiles of the 320 x 200 frame: A and B side by side with 64 columns in common, C far away and empty
CRAFT_CORNERS = [(0, 0), (64, 0), (192, 136)]
CRAFT_A = [  # (level, ix, iy, sides, cls, logit): boxes in A's pixels = full-frame pixels
    (0, 10, 1, (2, 1, 3, 1), 3, 1.0),        # (68, 4, 108, 20)    duplicate of B[0], lower score: suppressed
    (0, 11, 3, (1, 0.5, 4.5, 1.5), 5, 3.0),  # (84, 24, 128, 40)   ends at A's right edge: cut; loses to B[1], the whole armor at a lower score
    (0, 10, 6, (2, 1, 2, 1), 7, 1.5),        # (68, 44, 100, 60)   B[2] of another class lies on it: both kept
    (1, 2, 1, (2, 1, 2, 1), 2, 2.5),         # (8, 8, 72, 40)      a nested pair of one tile ...
    (0, 4, 2, (1, 1, 1, 1), 2, 2.0),         # (28, 12, 44, 28)    ... whose own NMS let both through: both kept
    (0, 13, 6, (1, 1, 1, 1), 9, 0.75),       # (100, 44, 116, 60)  exact score tie with B[3]: the lower tile wins
]
CRAFT_B = [  # boxes in B's pixels: full-frame x = local x + 64
    (0, 2, 1, (2, 1, 3, 1), 3, 2.0),         # (68, 4, 108, 20)
    (0, 3, 3, (1, 0.5, 8, 1.5), 5, 0.5),     # (84, 24, 156, 40)
    (0, 2, 6, (2, 1, 2, 1), 8, 1.0),         # (68, 44, 100, 60)
    (0, 5, 6, (1, 1, 1, 1), 9, 0.75),        # (100, 44, 116, 60)
    (0, 0, 4, (0.5, 1, 1, 1), 1, 1.0),       # (64, 28, 76, 44)    starts at B's left edge: cut, nothing covers it: kept with cut = 1
]


def run_crafted(w, heads):
    for s, h in enumerate(heads):
        w.write_head(h, s)
    w.run_post(0, len(heads))
    w.merge_tiles(0, len(heads))


def test_crafted_results_show_every_rule(blob):
    with weng(blob, full=FULL2, win=WIN2, net=WIN2, num_slots=3, max_det=9) as w:
        w.set_tiles(CRAFT_CORNERS)
        heads = [crafted_head(w, WIN2, CRAFT_A), crafted_head(w, WIN2, CRAFT_B), crafted_head(w, WIN2, [])]
        run_crafted(w, heads)
        lists, _ = slot_lists(w, 0, 3)
        assert [len(L["scores"]) for L in lists] == [6, 5, 0]                       # every crafted record came out of its tile's NMS; C is empty
        assert np.array_equal(lists[0]["boxes"][np.argsort(-lists[0]["scores"], kind="stable")][0], [84, 24, 128, 40])
        trace = check_merge(w, 0, CRAFT_CORNERS, FULL2, WIN2)
        box = {(t, i): tuple(lists[t]["boxes"][i]) for t in range(2) for i in range(len(lists[t]["scores"]))}
        tr = {box[(t["tile"], t["index"])] + (t["tile"],): t for t in trace}
        dup, part, whole = tr[(68, 4, 108, 20, 0)], tr[(84, 24, 128, 40, 0)], tr[(84, 24, 156, 40, 1)]
        assert dup["rule"] == "suppressed" and box[(1,) + dup["by"][1:]] == (68, 4, 108, 20) and dup["by"][0] == 1      # cross-tile duplicate
        assert part["cut"] == 1 and part["rule"] == "suppressed" and part["score"] > whole["score"] and whole["rule"] == "kept" and whole["cut"] == 0
        assert tr[(68, 44, 100, 60, 0)]["rule"] == tr[(68, 44, 100, 60, 1)]["rule"] == "kept"                       # different classes
        assert len(tr[(68, 44, 100, 60, 1)]["spared_other_class"]) == 1
        assert tr[(28, 12, 44, 28, 0)]["rule"] == "kept" and len(tr[(28, 12, 44, 28, 0)]["spared_same_tile"]) == 1    # same-tile nested pair
        tie_a, tie_b = tr[(100, 44, 116, 60, 0)], tr[(100, 44, 116, 60, 1)]
        assert tie_a["score"] == tie_b["score"] and tie_a["rule"] == "kept" and tie_b["rule"] == "suppressed"        # exact tie
        edge = tr[(64, 28, 76, 44, 1)]
        assert edge["cut"] == 1 and edge["rule"] == "kept"
        assert sum(t["rule"] == "kept" for t in trace) == 8 and cross_tile_suppressions(trace) == 3                   # 11 in, 3 suppressed
        # other parameters, live: nothing re-captured, the new pair read by the next merge
        g = w.debug_graph_count()
        w.set_tile_merge(1.0, 30.0)               # nothing exceeds its own smaller area: no suppression at all; margin 30: more cuts
        assert w.tile_merge == (1.0, 30.0)
        w.merge_tiles(0, 3)
        trace2 = check_merge(w, 0, CRAFT_CORNERS, FULL2, WIN2, 1.0, 30.0)
        assert [t["rule"] for t in trace2] == ["kept"] * 9 + ["cap"] * 2 and sum(t["cut"] for t in trace2) > sum(t["cut"] for t in trace)
        w.set_tile_merge(0.3, 0.0)                # margin 0: a box that ends ON the edge is not cut (128 > 128 is false)
        w.merge_tiles(0, 3)
        trace3 = check_merge(w, 0, CRAFT_CORNERS, FULL2, WIN2, 0.3, 0.0)
        assert sum(t["cut"] for t in trace3) == 0 and cross_tile_suppressions(trace3) == 3
        assert w.debug_graph_count() == g
        for bad in [(0.0, 2.0), (1.5, 2.0), (float("nan"), 2.0), (0.5, -1.0), (0.5, float("nan"))]:
            with pytest.raises(capi.IrmvError):
                w.set_tile_merge(*bad)
        assert w.tile_merge == (np.float32(0.3), 0.0)


def test_merge_at_capacity(blob):
    """16 tiles x max_det 256, every tile full: 4096 records enter, the sort and the walk run at their largest.  A decoy head
    (no step produces it) with two classes lit on all 128 anchors of level 0 and 8 x 8 boxes that touch without overlapping:
    256 detections per tile.  The 4 x 4 grid's columns are 64 pixels apart, so neighbouring tiles see the same boxes."""
    corners, nx, ny = capi.tile_grid(FULL2, WIN2, (64, 18), net_size=WIN2[0], net_height=WIN2[1])
    assert (nx, ny) == (4, 4)
    with weng(blob, full=FULL2, win=WIN2, net=WIN2, num_slots=16, max_det=256) as w:
        w.set_tiles(corners)
        A, no = w.num_anchors, w.head_channels
        nc, n0 = no - 72, dc.level_sizes(*WIN2)[0]
        assert n0 == 128
        rng = np.random.default_rng(7)
        for s in range(16):
            h = dc.decoy_head(A, no, nc, 100 + s)
            h[:n0, :64] = dc.OFF_BIN
            h[:n0, 0:64:16] = 0.0
            h[:n0, 1:64:16] = 0.0                       # every side half a stride
            h[:n0, 64 + (s // 4) % 3] = rng.uniform(0.5, 3.0, n0).astype(np.float32)   # one class per row of tiles: neighbours duplicate
            h[:n0, 64 + 5] = np.float32(1.0 + 0.125 * (s % 4))     # ties inside a tile and across tiles
            w.write_head(h, s)
        w.run_post(0, 16)
        w.merge_tiles(0, 16)
        recs, n_in = w.tile_results_raw(0)
        assert n_in == 4096 and len(recs) == 256
        trace = check_merge(w, 0, corners, FULL2, WIN2)
        assert cross_tile_suppressions(trace) > 0 and sum(t["rule"] == "cap" for t in trace) > 0


# ---- 3a. the merge ladder (tests/tile_ladder.py) ---------------------------------------------------------------------------------
# Which part of tile_merge_kernel each case reaches, and why, is stated in tests/tile_ladder.py; tests/test_tile_ladder.py
# asserts the same reach conditions on the host alone.  Wall time per test on the MI355X (two runs; most of it is the host
# reference's walk): suppressors 0.65 - 0.76 s per max_det, ties on the boundary 0.06 - 0.16 s, input counts 0.23 s (one tile),
# 0.32 - 0.40 s (two), 0.34 - 0.45 s for each of the four sixteen-tile tests.  (Tried once on a build whose walk ignored
# register 3 of the kept list: the three suppressor tests fail, test_merge_at_capacity passes.)


def ladder_merge(w, tile_recs, corners, ios_thr=0.5, edge_margin=0.0):
    """Crafted tiles through decode + NMS + merge; -> (lists, kept, trace) of the reference on the GPU's own tile lists, after
    check_merge has compared the kernel's list with it."""
    run_crafted(w, [crafted_head(w, WIN2, r) for r in tile_recs])
    lists, _ = slot_lists(w, 0, len(corners))
    assert [len(L["scores"]) for L in lists] == [min(len(r), w.max_det) for r in tile_recs]   # every crafted record came out of its tile's NMS, up to its max_det
    kept, trace = tiles.merge(lists, corners, WIN2, FULL2, ios_thr, edge_margin, w.max_det)
    return lists, kept, trace


@pytest.mark.parametrize("max_det", [256, 255, 250])
def test_merge_suppressors_in_every_register_and_lane(blob, max_det):
    """240 records of tile 0 kept first, each the twin of one of tile 1's: the suppressors sit at kept positions 0 .. 239, in
    all four registers of the walk and every lane (asserted from the reference's trace, then the kernel is compared); then
    the same tiles with the scores swapped: tile 1 alone fills the list."""
    with weng(blob, full=FULL2, win=WIN2, net=WIN2, num_slots=2, max_det=max_det) as w:
        w.set_tiles(tl.SUP_CORNERS)
        w.set_tile_merge(0.5, 0.0)
        lists, kept, trace = ladder_merge(w, tl.suppressor_tiles(), tl.SUP_CORNERS)
        blocks, residues = tl.suppressor_reach(kept, trace)
        assert len(kept) == max_det and blocks == [0, 1, 2, 3] and residues == list(range(64))
        assert sum(t["cut"] for t in trace) == 0
        assert check_merge(w, 0, tl.SUP_CORNERS, FULL2, WIN2, 0.5, 0.0) == trace
        lists, kept, trace = ladder_merge(w, tl.suppressor_tiles(swap=True), tl.SUP_CORNERS)
        assert len(kept) == max_det and all(k[0] == 1 for k in kept)
        check_merge(w, 0, tl.SUP_CORNERS, FULL2, WIN2, 0.5, 0.0)


def test_merge_tied_scores_on_the_register_boundary(blob):
    """Equal scores inside a tile and across the two, on kept positions 62 .. 65: the order is (tile, index), the 64th kept
    record (last lane of register 0) and the 65th (first lane of register 1) each suppress a twin."""
    with weng(blob, full=FULL2, win=WIN2, net=WIN2, num_slots=2, max_det=256) as w:
        w.set_tiles(tl.SUP_CORNERS)
        w.set_tile_merge(0.5, 0.0)
        lists, kept, trace = ladder_merge(w, tl.tied_boundary_tiles(), tl.SUP_CORNERS)
        score = lambda k: lists[k[0]]["scores"][k[1]]
        assert len(kept) == 66 and [k[0] for k in kept[62:66]] == [0, 0, 1, 1]
        assert score(kept[61]) > score(kept[62]) == score(kept[63]) == score(kept[64]) == score(kept[65])
        pos = {(t, i): j for j, (t, i, _) in enumerate(kept)}
        assert sorted(pos[tuple(t["by"])] for t in trace if t["rule"] == "suppressed") == [63, 64]
        check_merge(w, 0, tl.SUP_CORNERS, FULL2, WIN2, 0.5, 0.0)


@pytest.mark.parametrize("count,lo,hi", [(1, 0, 256), (2, 0, 512), (16, 0, 257), (16, 1023, 1025), (16, 2047, 2049), (16, 4095, 4096)])
def test_merge_input_counts(blob, count, lo, hi):
    """n_in = 0 .. 5 and one rung either side of every size of the sort (P = 64 .. 4096), the records spread over 1, 2 and 16
    tiles with empty tiles first, in the middle and last; ios_thr 1.0: nobody suppresses anybody, min(n_in, max_det) are kept.
    (Sixteen tiles in four tests: none walks more than three large lists through the host reference.)"""
    corners, nx, ny = capi.tile_grid(FULL2, WIN2, (64, 18), net_size=WIN2[0], net_height=WIN2[1])
    assert (nx, ny) == (4, 4)
    corners = corners[:count]
    ladder = [n for n in tl.input_counts(count) if lo <= n <= hi]
    assert len(ladder) >= 2
    with weng(blob, full=FULL2, win=WIN2, net=WIN2, num_slots=count, max_det=256) as w:
        w.set_tiles(corners)
        w.set_tile_merge(1.0, 0.0)
        seen_empty = set()
        for n_in in ladder:
            per = tl.spread(n_in, count)
            seen_empty |= {t for t in range(count) if per[t] == 0 and n_in > 0}
            run_crafted(w, [crafted_head(w, WIN2, tl.isolated(k, 100 * count + t)) for t, k in enumerate(per)])
            recs, got_in = w.tile_results_raw(0)
            assert got_in == n_in and len(recs) == min(n_in, 256), (count, n_in)
            trace = check_merge(w, 0, corners, FULL2, WIN2, 1.0, 0.0)
            assert len(trace) == n_in and cross_tile_suppressions(trace) == 0
        want = {0, 8, 15} if count == 16 and lo <= 13 * 256 else ({0, 1} if count == 2 else set())
        assert want <= seen_empty, (count, lo, seen_empty)      # (small n_in leave further tiles empty)


# ---- 4. launch forms -------------------------------------------------------------------------------------------------------------
def test_launch_forms_and_moving_tiles(wblob):
    frame, other = frame_of(12), frame_of(61)
    moved = [(5, 37), (31, 40), (66, 73), (13, 9)]
    with weng(wblob, num_slots=5) as w:
        def step(what, corners, **kw):
            w.submit_tiles(0, 1, 4, **kw)
            w.wait_slots(1, 4)
            n = 0
            for t, org in enumerate(corners):
                n += same_results(snapshot(w, 1 + t, False), reference(wblob, frame, org, tag="f12"), org, (what, t))
            check_merge(w, 1, corners, FULL, WIN)
            assert n > 0, what
        for s in range(1, 5):
            w.get_src_image_buffer(s)[:] = other
        w.get_src_image_buffer(0)[:] = frame
        w.set_tiles(CORNERS4, first=1)
        g0 = w.debug_graph_count()
        step("sync", CORNERS4)
        g1 = w.debug_graph_count()
        assert g1 == g0 + 1
        step("sync again", CORNERS4)
        assert w.debug_graph_count() == g1              # a second submit captures nothing
        w.set_tiles(moved, first=1)
        step("moved", moved)                            # ... nor does moving the tiles, and the results follow the corners
        assert w.debug_graph_count() == g1
        step("async upload", moved, async_upload=True)
        g2 = w.debug_graph_count()
        assert g2 == g1 + 1                             # (the graph without the upload node)
        w.get_src_image_buffer(0)[:] = 0                # a device-resident frame: the pinned slot is not read
        _hip_memcpy_h2d(w.src_device_ptr(0), frame)
        step("device frame", moved, h2d=False)
        assert w.debug_graph_count() == g2              # (the same graph)
        w.get_src_image_buffer(0)[:] = frame
        w.set_tiles(CORNERS4, first=1)
        step("sync, back", CORNERS4)
        assert w.debug_graph_count() == g2
        # a later upload into the frame's slot waits for the tiled step: an ordinary step of slot 0 behind it sees its own frame
        w.submit_tiles(0, 1, 4)
        w.get_src_image_buffer(0)[:] = frame            # (unchanged: the tiled step may still be reading it)
        w.set_window(31, 40, slot=0)
        w.detect(0)
        assert same_results(snapshot(w, 0, False), reference(wblob, frame, (31, 40), tag="f12"), (31, 40), "slot 0 behind") > 0
        w.wait_slots(1, 4)
        check_merge(w, 1, CORNERS4, FULL, WIN)


def test_tiled_and_single_slot_steps_order_across_compute_streams(wblob):
    """Five slots give two compute streams: single-slot steps of slots 1 and 3 ride stream 1, tiled steps stream 0.  Submitted
    back to back with no wait in between, the later step of a slot is ordered behind the earlier one on the other stream."""
    a, b = frame_of(12), frame_of(61)
    with weng(wblob, num_slots=5) as w:
        w.get_src_image_buffer(0)[:] = a
        for s in range(1, 5):
            w.get_src_image_buffer(s)[:] = b
        w.set_tiles(CORNERS4, first=1)
        g0 = w.debug_graph_count()
        # 1. the tiled step runs behind slot 1's ordinary step and overwrites it
        w.submit(1, 1, async_upload=True)
        w.submit_tiles(0, 1, 4)
        w.wait_slots(1, 4)
        solved = 0
        for t, org in enumerate(CORNERS4):
            solved += same_results(snapshot(w, 1 + t, False), reference(wblob, a, org, tag="f12"), org, ("tiles behind slot 1", t))
        check_merge(w, 1, CORNERS4, FULL, WIN)
        assert solved > 0
        g1 = w.debug_graph_count()
        assert g1 == g0 + 2                             # slot 1's step without an upload node, the tiled step with one
        # 2. slot 3's ordinary step waits for the tiled one before its upload and crop replace the slot's frames
        w.submit_tiles(0, 1, 4)
        w.submit(3, 1, async_upload=True)
        w.wait_slots(3, 1)
        org = CORNERS4[2]
        assert same_results(snapshot(w, 3, False), reference(wblob, b, org, tag="f61"), org, "slot 3 behind the tiles") > 0
        w.wait_slots(1, 4)
        assert w.debug_graph_count() == g1 + 1          # slot 3's step; the tiled step captured nothing again


# ---- 5. Bayer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["bilinear", "mhc"])
def test_bayer_tiles_are_bayer_windows(wblob, algo):
    """One demosaic of frame_slot's raw frame feeds every tile: each is the plain Bayer window engine's step at its corner."""
    full, pattern = (322, 202), "GRBG"
    corners = [(0, 0), (66, 74), (31, 41)]
    raw = bayer.mosaic(frame_of(17, full), pattern)
    junk = bayer.mosaic(frame_of(18, full), pattern)
    solved = 0
    with weng(wblob, full=full, src_format=pattern, bayer_demosaic=algo, num_slots=4) as t, \
            weng(wblob, full=full, src_format=pattern, bayer_demosaic=algo) as b:
        for s in range(4):
            t.get_src_image_buffer(s)[:] = raw if s == 3 else junk
        b.get_src_image_buffer()[:] = raw
        t.set_tiles(corners)
        t.submit_tiles(3, 0, 3)
        t.wait_slots(0, 3)
        for i, org in enumerate(corners):
            b.set_window(*org)
            b.detect()
            got, ref = snapshot(t, i), snapshot(b, 0)
            same_tensors(got, ref)
            solved += same_results(got, ref, (0, 0), (algo, org))       # both already carry the corner
        check_merge(t, 0, corners, full, WIN)
    assert solved > 0


# ---- 6. real size, classical point source ------------------------------------------------------------------------------------
def test_real_size_classical_tiles(blob, rm_test_image):
    """rm_test.jpg, 1280 x 1024 as a 3 x 3 grid of 640 x 512 windows at the sensor's resolution, the classical point source:
    each tile against the window engine.  (Crafted finals as in test_gpu_window: 192 x 192 boxes of level 2 on a grid.)"""
    full, win, rot = (1280, 1024), (640, 512), False
    lit = {0: ("bias", dc.dark_bias(14)), 1: ("bias", dc.dark_bias(14)), 2: ("bias", dc.two_tied_bias(14))}
    b = dc.craft(blob, cls=lit, box=("bias", dc.dfl_bias(3)))
    kw = dict(point_source=capi.POINTS_CLASSICAL, rotate180=rot, armor_size=capi.ARMOR_LARGE)
    corners, nx, ny = capi.tile_grid(full, win, 128, rotate180=rot, net_size=win[0], net_height=win[1])
    assert (nx, ny) == (3, 3)
    armors = 0
    with weng(b, full, win, win, num_slots=10, **kw) as t, weng(b, full, win, win, **kw) as w:
        t.get_src_image_buffer(0)[:] = rm_test_image
        w.get_src_image_buffer()[:] = rm_test_image
        t.set_tiles(corners, first=1)
        t.submit_tiles(0, 1, 9)
        t.wait_slots(1, 9)
        for i, org in enumerate(corners):
            w.set_window(*org)
            w.detect()
            got, ref = snapshot(t, 1 + i, False), snapshot(w, 0, False)
            same_results(got, ref, (0, 0), org)
            armors += sum(d["ints"][3] == 1 and d["ints"][5] == 2 for d in got["dets"])
        trace = check_merge(t, 1, corners, full, win)
        assert armors > 0 and len(trace) > 0


# ---- 7. refusals on a live engine --------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(wblob):
    frame = frame_of(12)
    with peng(wblob, num_slots=2) as p:
        L, h = p._L, p._h
        assert L.irmv_engine_submit_tiles(h, 0, 0, 2, capi.SUBMIT_H2D) == capi.ERR_ARG and b"no window" in L.irmv_last_error()
        assert L.irmv_engine_merge_tiles(h, 0, 2) == capi.ERR_ARG and b"no window" in L.irmv_last_error()
        n = C.c_int(0)
        assert L.irmv_engine_tile_results(h, 0, None, 0, C.byref(n), None) == capi.ERR_ARG
        assert L.irmv_engine_set_tile_merge(None, 0.5, 2.0) == capi.ERR_ARG
    with weng(wblob, num_slots=18) as w:
        L, h = w._L, w._h
        g0 = w.debug_graph_count()
        n = C.c_int(0)
        assert L.irmv_engine_tile_results(h, 0, None, 0, C.byref(n), None) == capi.ERR_ARG and b"no tiled step" in L.irmv_last_error()
        for first, count in [(0, 0), (0, 17), (0, -1), (-1, 2), (17, 2)]:
            assert L.irmv_engine_submit_tiles(h, 0, first, count, capi.SUBMIT_H2D) == capi.ERR_ARG, (first, count)
            assert L.irmv_engine_merge_tiles(h, first, count) == capi.ERR_ARG, (first, count)
        for frame_slot in (-1, 18):
            assert L.irmv_engine_submit_tiles(h, frame_slot, 0, 2, capi.SUBMIT_H2D) == capi.ERR_ARG and b"frame_slot" in L.irmv_last_error()
        w.set_view("frame", slot=1)
        assert L.irmv_engine_submit_tiles(h, 0, 0, 2, capi.SUBMIT_H2D) == capi.ERR_ARG and b"frame view" in L.irmv_last_error()
        assert L.irmv_engine_merge_tiles(h, 0, 2) == capi.ERR_ARG and b"frame view" in L.irmv_last_error()
        assert L.irmv_engine_set_view(h, 0, 2) == capi.ERR_ARG          # tiling is a way of submitting, not a view
        w.set_view("window", slot=1)
        assert L.irmv_engine_tile_results(h, 0, None, 0, C.byref(n), None) == capi.ERR_ARG      # still: no merge has run
        assert w.debug_graph_count() == g0                              # nothing was captured ...
        # ... and ordinary steps of the same slots give the window engine's bits from their own frames
        orgs = [(0, 0), (66, 73)]
        for s, org in enumerate(orgs):
            w.get_src_image_buffer(s)[:] = frame
            w.set_window(*org, slot=s)
        w.submit(0, 2)
        w.wait()
        solved = 0
        for s, org in enumerate(orgs):
            solved += same_results(snapshot(w, s, False), reference(wblob, frame, org, tag="f12"), org, ("submit", s))
        w.detect(1)
        solved += same_results(snapshot(w, 1, False), reference(wblob, frame, orgs[1], tag="f12"), orgs[1], "detect")
        assert solved > 0


# ---- 8. the C++ facade ---------------------------------------------------------------------------------------------------------
def test_facade_detect_tiles_is_the_python_mirror(tmp_path, wblob):
    """tests/cpp/tiles_facade_test.cpp: a YoloEngine built with tile_overlap searches the frame in its buffer; its merged boxes
    are, bit for bit, what the Python mirror's tiled step on the same grid returns."""
    from test_tiles import facade_exe
    frame = frame_of(12)
    (tmp_path / "model.irmw").write_bytes(wblob)
    frame.tofile(tmp_path / "frame.bin")
    out = subprocess.run([facade_exe(build=False), str(tmp_path / "model.onnx"), str(tmp_path / "frame.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tiles 4 grid 2 2" in out.stdout
    got = [tuple(int(v, 16) for v in m[:5]) + tuple(int(v) for v in m[5:])
           for m in re.findall(r"det \d+ (\w+) (\w+) (\w+) (\w+) (\w+) (\d+) tile (\d+) index (\d+) cut (\d+)", out.stdout)]
    with weng(wblob, num_slots=5) as w:
        assert w.tile_grid((190, 55)) == (CORNERS4, 2, 2)
        w.get_src_image_buffer(0)[:] = frame
        w.set_tiles(CORNERS4, first=1)
        w.submit_tiles(0, 1, 4)
        w.wait_slots(1, 4)
        recs, _ = w.tile_results_raw(1)
    ref = [tuple(int(v) for v in np.array(list(r.det.xyxy) + [r.det.score], np.float32).view(np.uint32)) + (r.det.class_id, r.tile, r.index, r.cut) for r in recs]
    assert len(ref) > 0 and got == ref
    assert int(re.search(r"found (\d+) records (\d+)", out.stdout).group(1)) == len(ref) and re.search(r"again \d+", out.stdout)
