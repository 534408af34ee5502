"""A zoo of hard shapes for the classical light extraction (contours, minimum-area rectangles, gating).

Deterministic, numpy only (scipy.ndimage.gaussian_filter for the smoothed noise).  Every shape is a small binary image
with a name; `build_zoo` packs them into 1280 x 1024 frames (foreground (255, 255, 255) on 0) and lists the boxes to
test.  Most boxes are exactly one shape's own rectangle, so the ROI's content is the shape's mask; the `roi` group adds
fractional, cutting, outside and whole-frame boxes on the same frames.

Groups: topology, scan, roi, big, caps, gate, threshold, random.  Only boxes of the `caps` group may exceed a limit of
the kernel (`Case.cap` says which one they are BUILT to exceed; the tests predict the verdict from the oracle's counts).

What the zoo cannot reach: a contour of 5 or more points that are all collinear.  CHAIN_APPROX_SIMPLE emits a point
only where the direction changes, so a line comes out as its two ends; the collinear branch of the rectangle (h == 2)
is checked on min_area_rect directly (tests/test_light_shapes.py)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
from scipy import ndimage

W, H = 1280, 1024
SCAN_COLUMNS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513)   # padded columns: block and chunk edges
EDGE_SIZES = (1, 2, 61, 62, 63, 64, 65, 66, 253, 254, 255, 256, 257, 258)


@dataclass
class Case:
    name: str
    group: str
    frame: int
    box: tuple                   # xyxy, float
    cap: Optional[str] = None    # 'contours' | 'points' | 'pool': built to exceed that limit


def label_bytes(rw, rh):
    """Bytes of a ROI's padded label image as the kernel reserves them (k_light.hip label_bytes)."""
    return ((rw + 2) * (rh + 2) + 15) & ~15


# ---- shapes -----------------------------------------------------------------------------------------------------------
def _z(h, w):
    return np.zeros((h, w), bool)


def pad(m, p=1):
    return np.pad(m, p)


def ring(n, t=1):
    m = np.ones((n, n), bool)
    m[t:n - t, t:n - t] = False
    return m


def ring_dot(n=7, t=1):
    m = ring(n, t)
    m[n // 2, n // 2] = True
    return m


def nested3(t=1):
    """ring, a second ring in its hole, a dot in that one's hole"""
    m = ring(8 * t + 5, t)
    m[2 * t:-2 * t, 2 * t:-2 * t] |= ring(4 * t + 5, t)
    m[4 * t + 2, 4 * t + 2] = True
    return m


def diag_touch():
    m = _z(6, 6)
    m[0:3, 0:3] = True
    m[3:6, 3:6] = True
    return m


def diag_chain(n=9, anti=False):
    m = np.eye(n, dtype=bool)
    return m[:, ::-1] if anti else m


def hline(n=9):
    return np.ones((1, n), bool)


def vline(n=9):
    return np.ones((n, 1), bool)


def plus(n=9):
    m = _z(n, n)
    m[n // 2, :] = True
    m[:, n // 2] = True
    return m


def xshape(n=9):
    return diag_chain(n) | diag_chain(n, True)


def tshape(n=9):
    m = _z(n, n)
    m[0, :] = True
    m[:, n // 2] = True
    return m


def spiral(n=17):
    """one-pixel-wide rectangular spiral, gaps one pixel wide"""
    m = _z(n, n)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    m[y0, x0:x1 + 1] = True
    while True:
        m[y0:y1 + 1, x1] = True
        if x1 - x0 < 2:
            break
        m[y1, x0:x1 + 1] = True
        y0 += 2
        if y1 - y0 < 0:
            break
        m[y0:y1 + 1, x0] = True
        x1 -= 2
        if x1 - x0 < 2:
            break
        m[y0, x0:x1 + 1] = True
        y1 -= 2
        x0 += 2
    return m


def checkerboard(h=9, w=11):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


def comb(teeth=5, length=5, k=0):
    """back of one pixel, teeth down; k quarter turns"""
    m = _z(length + 1, 2 * teeth - 1)
    m[0, :] = True
    m[:, ::2] = True
    return np.rot90(m, k)


def c_with_inside(k=0, closed=False, t=1):
    """a "C" opening to the right (k quarter turns; closed: an "O") with a 2 x 2 component in its middle"""
    n = 9 + 2 * t
    m = ring(n, t)
    if not closed:
        m[t + 1:n - t - 1, n - t:] = False
    m[n // 2 - 1:n // 2 + 1, n // 2 - 1:n // 2 + 1] = True
    return np.rot90(m, k)


def corner_pixels(h=7, w=9):
    m = _z(h, w)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    return m


def disc(rx, ry=None):
    ry = rx if ry is None else ry
    yy, xx = np.mgrid[-ry:ry + 1, -rx:rx + 1]
    return (xx / (rx + 0.25)) ** 2 + (yy / (ry + 0.25)) ** 2 <= 1.0


def ngon(n, R, phase=0.1):
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
    m = np.ones(xx.shape, bool)
    for k in range(n):
        a = phase + 2 * np.pi * k / n
        m &= xx * np.cos(a) + yy * np.sin(a) <= R * np.cos(np.pi / n)
    return m


def diamond(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return np.abs(xx) + np.abs(yy) <= r


def notched(m, y, x):
    """one border pixel less: the hull keeps its four vertices (every edge ties), the contour gets more than four points"""
    assert m[y, x]
    m = m.copy()
    m[y, x] = False
    return m


def staircase(steps, run=2, thick=3):
    m = _z(steps * run + thick, steps * run + run)
    for s in range(steps):
        m[s * run:s * run + thick, s * run:s * run + 2 * run] = True
    return m


def sawtooth(w, period=4, body=4):
    """a band whose upper and lower edges are triangle waves: about 4 contour points per period"""
    a = period // 2
    x = np.arange(w)
    tri = np.abs((x % period) - a)
    m = _z(2 * a + body + 1, w)
    for xi in range(w):
        m[tri[xi]:a + body + 1 + tri[xi], xi] = True
    return m


def bar(w=4, h=16):
    """an upright light: corners cut, so the contour has 8 points (a plain rectangle has 4 and is never measured)"""
    m = np.ones((h, w), bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = False
    return m


def blob_fail(n=6):
    """a contour of more than 4 points that fails the light gate (as wide as it is long)"""
    m = np.ones((n, n), bool)
    m[0, 0] = m[-1, -1] = False
    return m


def isolated_grid(count, cols=64):
    """`count` isolated pixels, every other column and row"""
    rows = (count + cols - 1) // cols
    m = _z(2 * rows - 1, 2 * cols - 1)
    for i in range(count):
        m[2 * (i // cols), 2 * (i % cols)] = True
    return m


TOPOLOGY = [
    ("ring", lambda: ring(7)), ("ring_thick", lambda: ring(9, 2)), ("ring_dot", lambda: ring_dot(7)), ("ring_dot_thick", lambda: ring_dot(11, 2)),
    ("nested3", lambda: nested3(1)), ("nested3_thick", lambda: nested3(2)), ("diag_touch", diag_touch),
    ("diag_chain", lambda: diag_chain(9)), ("anti_chain", lambda: diag_chain(9, True)), ("hline", hline), ("vline", vline),
    ("plus", plus), ("x", xshape), ("t", tshape), ("t_up", lambda: tshape()[::-1]), ("spiral", spiral), ("spiral_t", lambda: spiral(15).T.copy()),
    ("checkerboard", checkerboard), ("checkerboard_odd", lambda: ~checkerboard(8, 10)),
    ("comb_down", lambda: comb(k=0)), ("comb_left", lambda: comb(k=1)), ("comb_up", lambda: comb(k=2)), ("comb_right", lambda: comb(k=3)),
    ("c_right", lambda: c_with_inside(0)), ("c_up", lambda: c_with_inside(1)), ("c_left", lambda: c_with_inside(2)), ("c_down", lambda: c_with_inside(3)),
    ("c_right_thick", lambda: c_with_inside(0, t=2)), ("c_left_thick", lambda: c_with_inside(2, t=2)),
    ("o_inside", lambda: c_with_inside(0, closed=True)), ("o_inside_thick", lambda: c_with_inside(0, closed=True, t=2)),
    ("pixel", lambda: np.ones((1, 1), bool)), ("corner_pixels", corner_pixels), ("full", lambda: np.ones((6, 8), bool)),
    ("two_pixels_h", lambda: np.ones((1, 2), bool)), ("two_pixels_d", lambda: np.eye(2, dtype=bool)),
]


# ---- composer ---------------------------------------------------------------------------------------------------------
class Zoo:
    def __init__(self):
        self.masks = []          # bool [H, W] per frame
        self.colours = []        # (foreground, background) per frame
        self.cases = []
        self._shelf = None

    def new_frame(self, fg=(255, 255, 255), bg=(0, 0, 0)):
        self.masks.append(np.zeros((H, W), bool))
        self.colours.append((fg, bg))
        self._shelf = [2, 2, 0]      # x, y, shelf height
        return len(self.masks) - 1

    def image(self, f):
        fg, bg = self.colours[f]
        img = np.empty((H, W, 3), np.uint8)
        img[:] = np.array(bg, np.uint8)
        img[self.masks[f]] = np.array(fg, np.uint8)
        return img

    def place(self, name, group, mask, cap=None, box=True):
        """the mask's rectangle becomes a ROI of the current frame (2 pixels clear of every other one); -> (x, y)"""
        h, w = mask.shape
        assert w <= W - 4 and h <= H - 4, name
        x, y, sh = self._shelf
        if x + w + 2 > W:
            x, y, sh = 2, y + sh + 2, 0
        if y + h + 2 > H:
            self.new_frame(*self.colours[-1])
            x, y, sh = 2, 2, 0
        f = len(self.masks) - 1
        self.masks[f][y:y + h, x:x + w] = mask
        self._shelf = [x + w + 2, y, max(sh, h)]
        if box:
            self.cases.append(Case(name, group, f, (float(x), float(y), float(x + w), float(y + h)), cap))
        return x, y

    def add_box(self, name, group, f, box, cap=None):
        self.cases.append(Case(name, group, f, tuple(float(v) for v in box), cap))

    def frame_cases(self, f):
        return [c for c in self.cases if c.frame == f]


def _smooth(rng, h, w, sigma, thr=0.52):
    return ndimage.gaussian_filter(rng.random((h + 8, w + 8)), sigma)[4:-4, 4:-4] > thr


def _scan_mask(c, inside):
    """a 12-row ROI whose candidate start pixel sits on padded column c (ROI column c - 1), judged with state carried from
    blocks before it: outside a component followed earlier in the row (external), or inside a hollow one (not)"""
    m = _z(12, c + 40)
    x = c - 1
    if inside:
        m[1:11, 1:x + 12] = True
        m[3:9, 3:x + 10] = False            # hole from column 3 on: the last event before x is its left wall
        m[5, x] = True                      # a dot in the hole ...
        m[4:7, x + 3:x + 6] = plus(3)       # ... and a plus, same block or the next
        m[5, x + 20:x + 25:2] = True        # outside again, to the right: three starts in one row
    else:
        g = 3 if c < 127 or c % 2 else 70   # the component before it ends in the same block, the one before, or the chunk before
        m[3:8, 2:x - g] = True              # followed from row 3 on; ends g columns before x
        m[5, x] = True
        m[5:8, x + 2] = True
        m[5, x + 4:x + 14:2] = True         # five more separate starts right behind, one row
        m[9, x:x + 2] = True
    return m


def build_zoo(lds_image=40 * 1024, n_random=300, seed=7):
    """lds_image: the kernel's LDS label-image limit (capi.light_limits()), for the ROI sizes on both sides of it."""
    z = Zoo()
    rng = np.random.default_rng(seed)

    # topology: each shape with a one-pixel margin, flush with all four ROI borders, and in a roomy ROI off centre
    f_topo = z.new_frame()
    for name, fn in TOPOLOGY:
        m = fn()
        z.place(name, "topology", pad(m, 1))
        z.place(name + "_flush", "topology", m)
        z.place(name + "_room", "topology", np.pad(m, ((2, 5), (4, 1))))

    # the same frame in the colours on both sides of the threshold: gray 151 on gray 150
    topo_cases = z.frame_cases(f_topo)
    f_thr = z.new_frame((0, 255, 3), (0, 255, 0))
    z.masks[f_thr][:] = z.masks[f_topo]
    for c in topo_cases:
        z.add_box(c.name, "threshold", f_thr, c.box)
    z.add_box("whole_frame", "threshold", f_thr, (0, 0, W, H))

    # scan geometry
    z.new_frame()
    for c in SCAN_COLUMNS:
        z.place(f"scan_out_{c}", "scan", _scan_mask(c, False))
        z.place(f"scan_in_{c}", "scan", _scan_mask(c, True))
    for w in (62, 63, 64, 65, 126, 127, 128, 254, 255, 256, 257, 258, 510, 511, 512):
        m = _z(10, w)                        # the sentinel column w + 1 on a block edge: shapes flush with the right border
        m[0, :] = m[4, :] = True
        m[0:5, 0] = m[0:5, -1] = True
        m[2, w // 2] = True                  # inside the hollow frame: not external
        m[6:9, w - 3:] = True
        m[7, 0] = True
        m[9, w - 1] = True
        z.place(f"sentinel_{w}", "scan", m)
    m = _z(3, 200)
    m[0, 3:190:4] = True                     # 47 starts in one row, every block several
    m[2, 1:199:2] = True
    z.place("many_starts", "scan", m)

    # ROI geometry: block- and chunk-edge sizes, LDS against pool label images, awkward boxes
    f_roi = z.new_frame()
    for s in EDGE_SIZES:
        z.place(f"w{s}_h20", "roi", _smooth(rng, 20, s, 1.2))
    for s in EDGE_SIZES:
        z.place(f"w20_h{s}", "roi", _smooth(rng, s, 20, 1.2))
    for s in (1, 2, 63, 64, 65):
        z.place(f"sq{s}", "roi", _smooth(rng, s, s, 1.0, 0.5) | (s <= 2))
        z.place(f"sq{s}_full", "roi", np.ones((s, s), bool))
    z.new_frame()
    s = int(np.sqrt(lds_image)) - 2
    while label_bytes(s + 1, s + 1) <= lds_image:
        s += 1
    while label_bytes(s, s) > lds_image:
        s -= 1
    hh = lds_image // 256 - 2
    while label_bytes(254, hh) > lds_image:
        hh -= 1
    for name, (w, h) in (("lds_sq", (s, s)), ("pool_sq", (s + 1, s + 1)), ("lds_rect", (254, hh)), ("pool_rect", (254, hh + 1))):
        assert (label_bytes(w, h) <= lds_image) == name.startswith("lds")
        z.place(name, "roi", _smooth(rng, h, w, 2.5))
    # boxes that are not a shape's own rectangle, on the sparse ROI frame
    base = [c for c in z.frame_cases(f_roi) if c.name in ("w64_h20", "w257_h20", "w20_h64", "sq63", "sq65", "w2_h20", "w20_h1")]
    for c in base:
        x0, y0, x1, y1 = c.box
        z.add_box(c.name + "_frac", "roi", f_roi, (x0 + 0.3, y0 + 0.7, x1 - 0.2, y1 - 0.6))
        z.add_box(c.name + "_frac2", "roi", f_roi, (x0 - 0.9, y0 - 0.1, x1 + 0.99, y1 + 0.5))
        z.add_box(c.name + "_cut", "roi", f_roi, (x0 + (x1 - x0) // 2, y0 + 3, x1 + 9, y1 + 7))
        z.add_box(c.name + "_cut2", "roi", f_roi, (x0 - 5, y0 - 4, x0 + (x1 - x0) // 3 + 1, y0 + (y1 - y0) // 2 + 1))
    for i, b in enumerate([(-30.5, -20.25, 140.75, 90.5), (-5, 3, 70, 40), (1200.5, 990.3, 1400, 1100), (1279.2, 0, 1290, 50), (0, 1023.5, 300, 1024),
                           (-50, -50, -1, -1), (1280, 10, 1300, 20), (10, 1024, 20, 1030), (100, 100, 100, 150), (100.2, 100, 100.9, 150), (50, 60, 40, 70),
                           (0, 0, 1, 1), (1279, 1023, 1280, 1024), (0, 0, W, 23), (0, 0, 66, 300)]):
        z.add_box(f"odd_box_{i}", "roi", f_roi, b)

    # big contours: global-memory contour path, hulls of more than 64 and 128 edges, ties between all edges
    z.new_frame()
    for name, m in (("disc150", disc(150)), ("ellipse420x330", disc(420, 330)), ("ellipse90x200", disc(90, 200)), ("gon64", ngon(64, 120)),
                    ("gon65", ngon(65, 121)), ("gon128", ngon(128, 200)), ("square", np.ones((90, 90), bool)), ("square_cut", bar(90, 90)),
                    ("square_notch", notched(np.ones((90, 90), bool), 0, 45)), ("diamond", diamond(60)), ("diamond_notch", notched(diamond(60), 30, 90)), ("diamond_small", diamond(3)), ("staircase", staircase(200)), ("staircase_up", staircase(140)[::-1].copy()),
                    ("saw", sawtooth(600)), ("disc40_ring", disc(40) & ~np.pad(disc(30), 10))):
        z.place(name, "big", pad(m, 1))

    # caps
    z.new_frame()
    for n in (1023, 1024, 1025):
        z.place(f"contours_{n}", "caps", isolated_grid(n), cap="contours" if n > 1024 else None)
    z.saw_frame = len(z.masks) - 1           # the point-count cases are finished by finish_point_caps (they need a contour follower)
    z.saw_boxes = []
    for n in (4095, 4096, 4097):
        m = _z(3 * 12 + 40, 1200)
        for k in range(3):
            m[12 * k:12 * k + 9, :] = sawtooth(1200)
        x, y = z.place(f"points_{n}", "caps", m, cap="points" if n > 4096 else None)
        z.saw_boxes.append((n, x, y, m.shape))
    # the label pool runs out in box order: seven whole frames fit, the eighth does not, nor anything after it
    f_pool = z.new_frame()
    z.place("pool_content", "caps", pad(np.hstack([bar(), _z(16, 20), bar()]), 3), box=False)
    small = (0, 0, 60, 30)
    for i in range(7):
        z.add_box(f"pool_whole_{i}", "caps", f_pool, (0, 0, W, H))
    z.add_box("pool_small_fits", "caps", f_pool, small)
    z.add_box("pool_whole_7", "caps", f_pool, (0, 0, W, H), cap="pool")
    z.add_box("pool_small_late", "caps", f_pool, small, cap="pool")

    # gate and merge: a row of contours found left to right (same top row); G = a light, F = fails the gate, t = too few points
    z.new_frame()
    def row(seq):
        m = _z(18, 10 * len(seq) + 2)
        for i, k in enumerate(seq):
            s = {"G": bar(), "F": blob_fail(), "t": np.ones((2, 2), bool)}[k]
            m[1:1 + s.shape[0], 10 * i + 1:10 * i + 1 + s.shape[1]] = s
        return m
    for ra in range(4):
        for rb in range(4):
            ib = rb + 4 * ((ra + rb) % 2)
            ia = ib + 1 + ((ra - ib - 1) % 4)
            seq = ["F" if i % 3 else "t" for i in range(ia + 1 + (ra + 2 * rb) % 3)]
            seq[ia] = seq[ib] = "G"
            for i in range(0, ib, 2 + (ra + rb) % 2):      # more lights before them: 2 to 9 in all
                seq[i] = "G"
            z.place(f"merge_last{ra}_prev{rb}_" + "".join(seq), "gate", row(seq))
    for seq in ("", "F", "t", "FtF", "G", "FGF", "tGtt", "GG", "FGFG", "GtFG", "GFFFFG", "GGGGGGGGG", "FFFFFFFFG", "GFFFFFFFFFFFG"):
        z.place("lights_" + (seq or "none"), "gate", row(list(seq)) if seq else _z(6, 6))
    yy, xx = np.mgrid[0:70, 0:120]
    m = _z(70, 120)
    for cx, t in ((30.0, 8.0), (85.0, -11.0)):
        a = np.deg2rad(t)
        u, v = (xx - cx) * np.cos(a) + (yy - 35.0) * np.sin(a), -(xx - cx) * np.sin(a) + (yy - 35.0) * np.cos(a)
        m |= (np.abs(u) <= 4) & (np.abs(v) <= 24)
    z.place("tilted_pair", "gate", m)
    z.add_box("whole_frame", "roi", len(z.masks) - 1, (0, 0, W, H))      # on this frame the whole frame stays within the limits

    # random ROIs: smoothed noise at several scales (holes, nesting) and raw noise in ROIs small enough for the limits
    z.new_frame()
    for i in range(n_random):
        if i % 3 == 2:
            h, w = int(rng.integers(3, 40)), int(rng.integers(3, 40))
            m = rng.random((h, w)) < rng.uniform(0.3, 0.6)
            name = f"raw_{i}"
        else:
            h, w = int(rng.integers(8, 110)), int(rng.integers(8, 130))
            sigma = (0.7, 1.0, 1.5, 2.0, 3.0)[i % 5]
            m = _smooth(rng, h, w, sigma, float(rng.uniform(0.47, 0.55)))
            name = f"smooth{sigma}_{i}"
        z.place(name, "random", m)
    return z


def finish_point_caps(z, count_points):
    """Top the three sawtooth ROIs of the caps group up with isolated pixels (one contour point each) until
    count_points(mask) -- a contour follower's total for the ROI -- is exactly 4095, 4096 and 4097."""
    for n, x, y, (h, w) in z.saw_boxes:
        m = z.masks[z.saw_frame][y:y + h, x:x + w]
        m[37:, :] = False
        k = n - count_points(m)
        assert 0 < k <= 2 * 590, (n, k)      # the sawtooth bands stay below the target; two rows of pixels can make up for it
        xs = 2 * np.arange(k)
        m[38, xs[xs < 1180]] = True
        m[40, xs[xs >= 1180] - 1180] = True
        assert count_points(m) == n, (n, count_points(m))
    z.saw_boxes = []
