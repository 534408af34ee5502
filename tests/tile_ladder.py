"""Crafted tile contents for tile_merge_kernel (csrc/k_tiles.hip) and the host reference tiles.merge: records as
test_gpu_tiles.crafted_head takes them -- (level, ix, iy, sides, cls, logit) -- plus a host simulation of what a tile's own
decode + NMS makes of them, so that the constructions can be checked on tiles.merge without a GPU (tests/test_tiles.py).

Every record is one 8 x 8 cell of level 0 of the 128 x 64 net (16 x 8 anchors): all four sides half a stride, boxes touch
without overlapping, so a tile's NMS keeps every record and lists them by score.

What the kernel's walk holds where (k_tiles.hip:113 - :139): kept record j sits in lane j % 64 of register j / 64 (four
registers at max_det 256), `have = r * 64 + lane < nkept` guards the part of a register that is filled, and a new record
goes to register nkept >> 6, lane nkept & 63.  The sort's size is the power of two P >= n_in (:75).
"""
import numpy as np

WIN = (128, 64)
COLS, ROWS = 16, 8
HALF = (0.5, 0.5, 0.5, 0.5)
_F = np.float32


def cell(ix, iy, cls, logit):
    return (0, int(ix), int(iy), HALF, int(cls), float(_F(logit)))


def tile_list(recs, corner):
    """What irmv_engine_results returns for a tile whose head holds `recs` (cells only): its NMS keeps them all, in the order
    score descending, anchor ascending, class ascending; boxes in full-frame pixels.  Scores here are the logits' float32
    sigmoid -- the kernel's own exp differs in the last bits, the ORDER does not (the logits are >= 1e-3 apart or equal)."""
    order = sorted(recs, key=lambda r: (-r[5], r[2] * COLS + r[1], r[4]))
    fx, fy = _F(corner[0]), _F(corner[1])
    boxes = np.array([[_F(8 * r[1]) + fx, _F(8 * r[2]) + fy, _F(8 * r[1] + 8) + fx, _F(8 * r[2] + 8) + fy] for r in order], _F).reshape(-1, 4)
    scores = np.array([1.0 / (1.0 + np.exp(-np.float64(r[5]))) for r in order]).astype(_F)
    return dict(boxes=boxes, scores=scores, classes=np.array([r[4] for r in order], int))


# ---- suppressors in every register and lane ---------------------------------------------------------------------------------
SUP_CORNERS = [(0, 0), (8, 0)]          # tile 1's column c is tile 0's column c + 1


def suppressor_tiles(swap=False, seed=5):
    """Tile 0: both classes on the 120 cells of columns 1 .. 15 (240 records, the higher scores).  Tile 1: the same on all
    16 of its columns (256 records, the lower scores): its columns 0 .. 14 are exact full-frame duplicates of tile 0's records,
    each suppressed by its twin and nobody else -- the twin's kept position is its rank in tile 0, so the 240 suppressors
    fill kept positions 0 .. 239: all four registers, every lane.  The 16 records of column 15 have no twin; they sit among
    tile 1's lowest 64 scores, so the walk has met most twins before it fills max_det on them.  swap: tile 1 scores high."""
    rng = np.random.default_rng(seed)
    classes = (2, 9)
    hi, lo = (0.0, 2.0) if swap else (2.0, 0.0)
    p0 = rng.permutation(240)
    t0 = [cell(ix, iy, c, hi + 0.004 * p0[k]) for k, (ix, iy, c) in
          enumerate((ix, iy, c) for ix in range(1, COLS) for iy in range(ROWS) for c in classes)]
    ranks = np.empty(256, int)
    low = rng.permutation(64)
    ranks[240:] = low[:16]                                   # column 15: sixteen of the lowest 64 ranks
    ranks[:240] = rng.permutation(np.concatenate([low[16:], np.arange(64, 256)]))
    t1 = [cell(ix, iy, c, lo + 0.004 * ranks[k]) for k, (ix, iy, c) in
          enumerate((ix, iy, c) for ix in range(COLS) for iy in range(ROWS) for c in classes)]
    return [t0, t1]


def suppressor_reach(kept, trace):
    """(blocks, residues) of the kept positions that suppressed somebody: position // 64 and position % 64."""
    pos = {(t, i): j for j, (t, i, _) in enumerate(kept)}
    hit = [pos[tuple(t["by"])] for t in trace if t["rule"] == "suppressed"]
    return sorted({p // 64 for p in hit}), sorted({p % 64 for p in hit})


# ---- input counts -----------------------------------------------------------------------------------------------------------
def input_counts(count, max_det=256):
    """n_in of the ladder for `count` tiles: 0 .. 5 and one rung either side of every sort size, capped at count * max_det."""
    out = {0, 1, 2, 3, 4, 5}
    for P in (64, 256, 1024, 2048, 4096):
        out |= {P - 1, P, P + 1}
    cap = count * max_det
    return sorted({min(n, cap) for n in out if n - 1 <= cap})


def spread(n_in, count, max_det=256):
    """Per-tile record counts that sum to n_in: where they fit, the first, a middle and the last tile stay EMPTY (one tile:
    nothing to leave out; two: the first or the last, by n_in's parity)."""
    if count == 1:
        empty = set()
    elif count == 2:
        empty = {n_in & 1} if n_in <= max_det else set()
    else:
        empty = {0, count // 2, count - 1} if n_in <= (count - 3) * max_det else set()
    live = [t for t in range(count) if t not in empty]
    per = [0] * count
    for k, t in enumerate(live):
        per[t] = n_in // len(live) + (k < n_in % len(live))
    assert sum(per) == n_in and max(per) <= max_det
    return per


def isolated(k, seed):
    """k records on distinct (cell, class) pairs, distinct logits."""
    rng = np.random.default_rng([7, int(seed), int(k)])
    pick = rng.choice(COLS * ROWS * 14, k, replace=False)
    logit = 0.5 + 0.004 * rng.permutation(max(k, 1))[:k]
    return [cell((p // 14) % COLS, (p // 14) // COLS, p % 14, l) for p, l in zip(pick, logit)]


# ---- ties on a register boundary ----------------------------------------------------------------------------------------------
def tied_boundary_tiles():
    """62 distinct high records (31 per tile), then FIVE records at one logit: two of tile 0 (kept positions 62, 63), three of
    tile 1 -- the first a full-frame twin of tile 0's second (suppressed by position 63: the last lane of register 0), the
    other two kept at positions 64, 65 (the first lanes of register 1).  Behind them a weaker record of tile 0 that is the
    twin of position 64's.  Corners SUP_CORNERS; classes 4 everywhere a twin matters."""
    t0 = [cell(1 + k % 15, k // 15, 4, 2.0 + 0.01 * k) for k in range(31)]           # rows 0 .. 2
    t1 = [cell(k % 16, 5 + k // 16, 4, 2.005 + 0.01 * k) for k in range(31)]         # rows 5 .. 6: no twin of the above
    tie = 1.0
    t0 += [cell(3, 3, 4, tie), cell(6, 3, 4, tie)]                                   # positions 62, 63
    t1 += [cell(5, 3, 4, tie), cell(9, 3, 4, tie), cell(12, 3, 4, tie)]              # twin of t0's (6, 3); positions 64, 65
    t0 += [cell(10, 3, 4, 0.5)]                                                      # twin of t1's (9, 3): suppressed by position 64
    return [t0, t1]
