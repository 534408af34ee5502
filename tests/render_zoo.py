"""Mark records for the debug-image tests (tests/test_render.py on the host, tests/test_gpu_render.py on the GPU): plain
dicts with the four fields irmv_engine_render reads."""
import numpy as np

NAN, INF = float("nan"), float("inf")
TWO24 = 16777216.0


def det(xyxy=(NAN,) * 4, cls=0, kpts=(NAN,) * 8, valid=0):
    return dict(xyxy=tuple(float(v) for v in xyxy), class_id=int(cls), kpts=tuple(float(v) for v in kpts), armor_valid=int(valid))


def zoo(w, h):
    """Marks for a w x h frame: boxes inside, across every edge, wholly outside, zero-sized and negative; classes of both
    colours, UNKNOWN and out-of-range ones; overlapping boxes of both colours; armors that are degenerate, axis-aligned,
    diagonal across the whole frame (several tiles of the kernel); NaN, inf and 2^24 in xyxy and in kpts; armor_valid 0, -1."""
    return [
        det((2.9, 3.2, w - 4.5, h - 3.1), 0, (3.2, h - 4.0, 4.9, 2.1, w - 5.0, 3.0, w - 4.0, h - 5.5), 1),
        det((-5.7, -3.2, 6.0, 7.9), 7), det((w - 6.0, 4.0, w + 9.0, h + 3.0), 14, (w - 8.0, 9.0, w - 8.0, 2.0, w + 5.0, -4.0, w + 7.0, 12.0), 1),
        det((3.0, -8.0, 9.0, 2.0), 4), det((5.0, h - 3.0, 15.0, h + 6.0), 13),
        det((w + 3.0, 2.0, w + 9.0, 9.0), 3), det((5.0, 5.0, 5.0, 5.0), 12), det((12.0, 11.0, 7.0, 4.0), 5),
        det((-30.0, -30.0, -20.0, -25.0), 1), det((4.0, h + 2.0, 9.0, h + 8.0), 9),
        det((1.0, 8.0, 14.0, 15.0), 6), det((3.0, 9.0, 12.0, 14.0), 8),           # overlapping, both colours: the last one wins
        det((NAN, 1.0, 5.0, 5.0), 2), det((1.0, INF, 5.0, 5.0), 2), det((1.0, 1.0, TWO24, 5.0), 2), det((1.0, 1.0, 5.0, -TWO24), 2),
        det((0.0, 0.0, 3.0, 3.0), 99), det((6.0, 6.0, 9.0, 9.0), -1),
        det(kpts=(5.0, 5.0) * 4, valid=1),                                          # degenerate: four times one point
        det(kpts=(2.0, 12.0, 2.0, 2.0, w - 4.0, 2.0, w - 4.0, 12.0), valid=1),      # axis-aligned
        det(kpts=(-9.0, h - 2.0, 1.0, -6.0, w + 6.0, 1.0, w - 5.0, h + 5.0), valid=1),   # diagonal, across the edges
        det(kpts=(2.0, 12.0, 2.0, 2.0, NAN, 2.0, 20.0, 12.0), valid=1), det(kpts=(2.0, 12.0, 2.0, -INF, 9.0, 2.0, 20.0, 12.0), valid=1),
        det(kpts=(2.0, 12.0, 2.0, 2.0, 9.0, 2.0, TWO24, 12.0), valid=1),
        det(kpts=(4.0, 4.0, 4.0, 9.0, 9.0, 9.0, 9.0, 4.0), valid=0), det(kpts=(4.0, 4.0, 4.0, 9.0, 9.0, 9.0, 9.0, 4.0), valid=-1),
        det(kpts=(1.0e6, -3.0e6, 11.0, 7.0, TWO24 - 1, TWO24 - 1, 1 - TWO24, 9.0), valid=1),   # the largest coordinates that count
    ]


def shifted(dets, ox, oy):
    """The same marks in a frame whose origin lies at (-ox, -oy): what a window at corner (ox, oy) is handed.  Values that
    are no number, or whose sum is not exact in fp32, stay (they draw nothing either way)."""
    def mv(vals):
        out = []
        for i, v in enumerate(vals):
            s = np.float32(v) + np.float32(oy if i & 1 else ox)
            out.append(float(s) if np.isfinite(s) and abs(v) < 2.0 ** 20 else v)
        return tuple(out)
    return [dict(d, xyxy=mv(d["xyxy"]), kpts=mv(d["kpts"])) for d in dets]


def stacked(n, seed=0):
    """n records whose boxes, labels and armors all touch the 64 x 16 tile at the frame's origin."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        x1, y1 = rng.integers(0, 40), rng.integers(0, 12)
        x2, y2 = x1 + rng.integers(0, 24), y1 + rng.integers(0, 10)
        k = rng.integers(-4, 60, 8).astype(np.float64) * np.array([1, 0.3] * 4) + rng.random(8)
        out.append(det((x1 + 0.5, y1 + 0.25, x2 + 0.75, y2), i % 16, k, 1 if i % 3 else 0))
    return out
