"""The tile-merge ladder's constructions (tests/tile_ladder.py) on the host reference tiles.merge: what they are built to
reach is asserted here from the reference alone; tests/test_gpu_tiles.py asserts it again on the GPU's own tile lists and
compares the kernel.  No GPU."""
import pytest

import tile_ladder as tl
from irmv_detection_amd import tiles

FULL2 = (320, 200)


def merged(tile_recs, corners, max_det, ios_thr=0.5, edge_margin=0.0):
    lists = [{k: v[:max_det] for k, v in tl.tile_list(r, c).items()} for r, c in zip(tile_recs, corners)]   # a tile's own NMS stops at max_det too
    return tiles.merge(lists, corners, tl.WIN, FULL2, ios_thr, edge_margin, max_det)


@pytest.mark.parametrize("max_det", [256, 255, 250])
def test_suppressors_sit_in_every_register_and_lane(max_det):
    recs = tl.suppressor_tiles()
    assert [len(r) for r in recs] == [240, 256]
    kept, trace = merged(recs, tl.SUP_CORNERS, max_det)
    assert len(kept) == max_det and sum(t["cut"] for t in trace) == 0
    assert [k[0] for k in kept[:240]] == [0] * 240                         # tile 0 first: its ranks are the kept positions
    blocks, residues = tl.suppressor_reach(kept, trace)
    assert blocks == [0, 1, 2, 3] and residues == list(range(64))
    sup = [t for t in trace if t["rule"] == "suppressed"]
    assert len(sup) >= 192 and all(t["tile"] == 1 and t["by"][0] == 0 for t in sup)
    if max_det < 256:
        assert any(t["rule"] == "cap" for t in trace)


def test_swapped_scores_fill_from_tile_one():
    kept, trace = merged(tl.suppressor_tiles(swap=True), tl.SUP_CORNERS, 256)
    assert len(kept) == 256 and all(k[0] == 1 for k in kept)              # register 3 filled to its last lane by ONE tile
    assert sum(t["rule"] == "cap" for t in trace) == 240


def test_tied_scores_on_the_register_boundary():
    recs = tl.tied_boundary_tiles()
    kept, trace = merged(recs, tl.SUP_CORNERS, 256)
    lists = [tl.tile_list(r, c) for r, c in zip(recs, tl.SUP_CORNERS)]
    score = lambda k: lists[k[0]]["scores"][k[1]]
    assert score(kept[61]) > score(kept[62]) == score(kept[63]) == score(kept[64]) == score(kept[65])
    assert [k[0] for k in kept[62:66]] == [0, 0, 1, 1]                     # equal scores: the lower tile first, then the index
    pos = {(t, i): j for j, (t, i, _) in enumerate(kept)}
    sup = {(t["tile"], float(t["score"])): pos[tuple(t["by"])] for t in trace if t["rule"] == "suppressed"}
    assert sorted(sup.values()) == [63, 64]                                 # the last lane of register 0, the first of register 1
    assert len(kept) == 66 and len(trace) == 68


def test_input_counts_and_spreads():
    assert tl.input_counts(1) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256]
    assert tl.input_counts(2)[-3:] == [255, 256, 257]
    assert tl.input_counts(16) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
    for count in (1, 2, 16):
        for n in tl.input_counts(count):
            per = tl.spread(n, count)
            assert sum(per) == n and len(per) == count and max(per) <= 256
    assert tl.spread(65, 16)[0] == tl.spread(65, 16)[8] == tl.spread(65, 16)[15] == 0
    assert tl.spread(5, 2) == [5, 0] and tl.spread(4, 2) == [0, 4] and 0 not in tl.spread(4096, 16)
    for k in (0, 1, 5, 256):
        recs = tl.isolated(k, 3)
        assert len({(r[1], r[2], r[4]) for r in recs}) == k == len({r[5] for r in recs})
        kept, trace = merged([recs], [(0, 0)], 256, ios_thr=1.0)
        assert len(kept) == k
