"""Host reference of the tiled search (include/irmv_hip.h "tiled search"; csrc/k_tiles.hip, irmv_tile_grid).

`grid` is the tile grid the engine documents, `cut_flags` the seam cut, `merge` the merge of the tiles' result lists.
Everything the kernel computes in fp32 is computed here in numpy float32, one rounded operation at a time and in the same
order, so the two agree bit for bit.  Boxes are the full-frame values irmv_engine_results returns.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

MAX_TILES = 16          # IRMV_MAX_TILES
DEFAULT_IOS_THR = 0.5   # the usual default of sliced inference; not validated on a trained model (none exists here)
DEFAULT_EDGE_MARGIN = 2.0   # source pixels; likewise

_F = np.float32


def axis(F: int, w: int, ov: int) -> List[int]:
    """Corners of one axis: frame extent F, window extent w, least overlap 0 <= ov < w."""
    if not (1 <= w <= F) or not (0 <= ov < w):
        raise ValueError("need 1 <= w <= F and 0 <= ov < w")
    if w == F:
        return [0]
    n = -(-(F - ov) // (w - ov))
    return [(2 * i * (F - w) + (n - 1)) // (2 * (n - 1)) for i in range(n)]


def grid(frame: Tuple[int, int], window: Tuple[int, int], overlap) -> Tuple[List[Tuple[int, int]], int, int]:
    """-> (corners, nx, ny): row-major (x, y) corners in result coordinates, t = iy * nx + ix.  overlap: one number or
    (ox, oy).  Raises ValueError where irmv_tile_grid refuses (an overlap out of range, more than MAX_TILES tiles)."""
    ox, oy = (overlap, overlap) if np.ndim(overlap) == 0 else overlap
    xs, ys = axis(int(frame[0]), int(window[0]), int(ox)), axis(int(frame[1]), int(window[1]), int(oy))
    if len(xs) * len(ys) > MAX_TILES:
        raise ValueError(f"{len(xs)} x {len(ys)} tiles: more than {MAX_TILES}")
    return [(x, y) for y in ys for x in xs], len(xs), len(ys)


def cut_flags(boxes, corner: Tuple[int, int], window: Tuple[int, int], frame: Tuple[int, int], edge_margin: float) -> np.ndarray:
    """bool [n]: the box comes within edge_margin of an edge of its tile that is not an edge of the frame."""
    b = np.asarray(boxes, _F).reshape(-1, 4)
    (x0, y0), (ww, wh), (FW, FH), m = corner, window, frame, _F(edge_margin)
    cut = np.zeros(len(b), bool)
    if x0 > 0:
        cut |= b[:, 0] < _F(x0) + m
    if y0 > 0:
        cut |= b[:, 1] < _F(y0) + m
    if x0 + ww < FW:
        cut |= b[:, 2] > _F(x0 + ww) - m
    if y0 + wh < FH:
        cut |= b[:, 3] > _F(y0 + wh) - m
    return cut


def score_order(score) -> int:
    """The unsigned the merge sorts scores by (descending = ascending in its complement): order-preserving bits of the fp32."""
    u = int(np.asarray(score, _F).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def ios_gt(a, b, thr) -> bool:
    """inter > thr * min(area_a, area_b) in fp32, no division (the iou_gt pattern of oracle/orc_post.c)."""
    a, b, thr = np.asarray(a, _F), np.asarray(b, _F), _F(thr)
    iw = max(_F(0), min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(_F(0), min(a[3], b[3]) - max(a[1], b[1]))
    inter = _F(iw * ih)
    aa = _F(_F(a[2] - a[0]) * _F(a[3] - a[1]))
    ab = _F(_F(b[2] - b[0]) * _F(b[3] - b[1]))
    return bool(inter > _F(thr * min(aa, ab)))


def merge(lists: Sequence[dict], corners: Sequence[Tuple[int, int]], window: Tuple[int, int], frame: Tuple[int, int],
          ios_thr: float = DEFAULT_IOS_THR, edge_margin: float = DEFAULT_EDGE_MARGIN, max_det: int = 100):
    """The merge of the tiles' lists.  lists[t]: dict(boxes float32 [n, 4] full-frame xyxy, scores float32 [n], classes int [n])
    in the order the tile's NMS produced.  -> (kept, trace):
      kept   [(tile, index, cut)] in merge order, at most max_det
      trace  one dict per record in sort order: tile, index, cut, score, cls, rule ("kept", "suppressed", or "cap": the walk had
             stopped), by = the (tile, index) that suppressed it, and the kept records that overlapped it (ios_gt) without
             suppressing: spared_same_tile, spared_other_class."""
    recs = []
    for t, (L, c) in enumerate(zip(lists, corners)):
        b = np.asarray(L["boxes"], _F).reshape(-1, 4)
        cut = cut_flags(b, c, window, frame, edge_margin)
        for k in range(len(b)):
            recs.append(dict(tile=t, index=k, cut=int(cut[k]), score=_F(L["scores"][k]), cls=int(L["classes"][k]), box=b[k]))
    recs.sort(key=lambda r: (r["cut"], (~score_order(r["score"])) & 0xFFFFFFFF, r["tile"], r["index"]))
    kept, kept_recs, trace = [], [], []
    for r in recs:
        tr = dict(tile=r["tile"], index=r["index"], cut=r["cut"], score=r["score"], cls=r["cls"], rule="kept", by=None,
                  spared_same_tile=[], spared_other_class=[])
        trace.append(tr)
        if len(kept) >= max_det:
            tr["rule"] = "cap"
            continue
        for q in kept_recs:
            if not ios_gt(r["box"], q["box"], ios_thr):
                continue
            if q["tile"] == r["tile"]:
                tr["spared_same_tile"].append((q["tile"], q["index"]))
            elif q["cls"] != r["cls"]:
                tr["spared_other_class"].append((q["tile"], q["index"]))
            elif tr["by"] is None:
                tr["rule"], tr["by"] = "suppressed", (q["tile"], q["index"])
        if tr["rule"] == "kept":
            kept.append((r["tile"], r["index"], r["cut"]))
            kept_recs.append(r)
    return kept, trace
