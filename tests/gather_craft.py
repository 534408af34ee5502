"""Crafted candidate sets for the candidate gather (k_boxg.hip; tests/test_gpu_gather_craft.py): bitmaps somebody chose,
written over the engine's candidate bitmap, instead of whatever the class branch emits on the synthetic frames.

Everything here is on the CPU and imports nothing of the GPU side.

    maps        a candidate set of a launch is bool [B, H, W]: image, row, column of ONE Detect level
    sets        the named single-image sets (named_sets), seeded launches of an exact list length (random_launch) and the
                batch layouts (batch_layouts)
    bits        pack_bits / unpack_bits: the engine's bitmap words of one image, anchor = level base + y * W + x
    lists       lists_of: per image the count and the ascending list cand_list_kernel's list is a permutation of; permuted:
                the three orders a written list is run in
    reach       the candidate anchors a NaN impulse in the level's input must turn NaN: by index arithmetic (reach_formula)
                and from conv_ref on a written input (reach_conv)
    passes      how many passes of 2 x 16 candidates a launch of n candidates has, and the most a workgroup walks
"""
from __future__ import annotations

import numpy as np

import conv_ref

STRIDES = (8, 16, 32)
PASS = 32                        # candidates of a pass: two groups of 16 (k_boxg.hip GNG * 16)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
PERMUTATIONS = ("reversed", "shuffled", "sorted")


# ---- geometry ---------------------------------------------------------------------------------------------------------
def level_dims(net_w: int, net_h: int):
    """[(H, W)] of the three Detect levels."""
    return [(net_h // s, net_w // s) for s in STRIDES]


def anchor_bases(dims):
    """([base of level 0, 1, 2], number of anchors): levels in turn, each row-major."""
    hw = [h * w for h, w in dims]
    return [0, hw[0], hw[0] + hw[1]], sum(hw)


def launch_lengths(grids):
    """The list lengths a seeded launch is built for: 1 .. 65 around the group and pass sizes, and 2 * 32 * g +- 1 for every
    grid g (one candidate short of, and one past, two whole passes per workgroup)."""
    n = list(LENGTHS)
    for g in grids:
        n += [2 * PASS * g - 1, 2 * PASS * g + 1]
    return sorted(set(n))


def passes(n: int) -> int:
    return -(-n // PASS)


def passes_of_workgroup(n: int, grid: int, wg: int = 0) -> int:
    """Passes wg, wg + grid, ... below passes(n)."""
    return len(range(wg, passes(n), grid))


# ---- single-image sets --------------------------------------------------------------------------------------------------
def named_sets(H: int, W: int):
    """{name: bool [H, W]}: the sets that exist on an H x W map.  An edge set is one pixel of that edge that is no corner, the
    interior set one pixel at least two pixels from every border where the map has one, else one pixel off every border."""
    def one(*p):
        m = np.zeros((H, W), bool)
        for y, x in p:
            m[y, x] = True
        return m
    s = {"empty": one(), "corner_tl": one((0, 0)), "corner_tr": one((0, W - 1)), "corner_bl": one((H - 1, 0)), "corner_br": one((H - 1, W - 1))}
    if W >= 3:
        s["edge_top"], s["edge_bottom"] = one((0, W // 2)), one((H - 1, W // 2))
    if H >= 3:
        s["edge_left"], s["edge_right"] = one((H // 2, 0)), one((H // 2, W - 1))
    if H >= 3 and W >= 3:
        s["interior"] = one((H // 2, W // 2))
    s["neighbours"] = one((H // 2, W // 2), (H // 2 - 1 if H > 1 else 0, W // 2 - 1))      # diagonal 8-neighbours
    s["full"] = np.ones((H, W), bool)
    s["checkerboard"] = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    return s


def cheb(p, q) -> int:
    return max(abs(p[0] - q[0]), abs(p[1] - q[1]))


def leaves_map_on_two_sides(H, W, y, x, r=2) -> bool:
    """The (2 r + 1)^2 neighbourhood of (y, x) leaves the map past at least two of its four borders."""
    return (y - r < 0) + (y + r >= H) + (x - r < 0) + (x + r >= W) >= 2


# ---- launches -----------------------------------------------------------------------------------------------------------
def in_image(B, H, W, b, m):
    out = np.zeros((B, H, W), bool)
    out[b] = m
    return out


def random_launch(seed: int, B: int, H: int, W: int, n: int) -> np.ndarray:
    """bool [B, H, W] with exactly n candidates, drawn without replacement over the whole launch."""
    assert 0 <= n <= B * H * W, (n, B, H, W)
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.zeros(B * H * W, bool)
    m[rng.choice(B * H * W, size=n, replace=False)] = True
    return m.reshape(B, H, W)


def random_image(seed: int, H: int, W: int, n: int) -> np.ndarray:
    return random_launch(seed, 1, H, W, n)[0]


def batch_layouts(seed: int, B: int, H: int, W: int):
    """{name: bool [B, H, W]}.  `only63` / `only64` exist where the launch has that image.  `alternating`: counts 0, H W, 1, 0,
    H W, 1, ... with the single candidates at seeded, mostly distinct pixels; `every_other_empty`: a different seeded set
    of H W // 3 + 1 candidates on every even image, none on the odd ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    some = lambda k: random_image(int(rng.integers(1 << 30)), H, W, k)   # noqa: E731
    k = H * W // 3 + 1
    out = {"all_in_first": in_image(B, H, W, 0, some(k)), "all_in_last": in_image(B, H, W, B - 1, some(k))}
    for b in (63, 64):
        if b < B:
            out[f"only{b}"] = in_image(B, H, W, b, some(k))
    eo = np.zeros((B, H, W), bool)
    for b in range(0, B, 2):
        eo[b] = some(k)
    out["every_other_empty"] = eo
    alt = np.zeros((B, H, W), bool)
    for b in range(B):
        if b % 3 == 1:
            alt[b] = True
        elif b % 3 == 2:
            alt[b] = some(1)
    out["alternating"] = alt
    return out


# ---- bits and lists -------------------------------------------------------------------------------------------------------
def pack_bits(level_maps, dims) -> np.ndarray:
    """One image's bitmap words (uint32 [ceil(A / 32)]) from {level: bool [H, W]} (a level left out has no candidate)."""
    bases, A = anchor_bases(dims)
    bits = np.zeros(-(-A // 32) * 32, bool)
    for lv, m in level_maps.items():
        assert m.shape == tuple(dims[lv]), (lv, m.shape, dims[lv])
        bits[bases[lv]:bases[lv] + m.size] = m.reshape(-1)
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def unpack_bits(words, dims):
    """The inverse: {level: bool [H, W]} of all three levels."""
    bases, A = anchor_bases(dims)
    bits = np.unpackbits(np.asarray(words, "<u4").view(np.uint8), bitorder="little").astype(bool)
    assert not bits[A:].any()
    return {lv: bits[bases[lv]:bases[lv] + h * w].reshape(h, w) for lv, (h, w) in enumerate(dims)}


def lists_of(maps: np.ndarray):
    """(counts int32 [B], entries int32 [B, H W]): per image its candidate pixels y * W + x ascending, the rest 0."""
    B, H, W = maps.shape
    counts = maps.reshape(B, -1).sum(1).astype(np.int32)
    entries = np.zeros((B, H * W), np.int32)
    for b in range(B):
        entries[b, :counts[b]] = np.flatnonzero(maps[b])
    return counts, entries


def permuted(counts, entries, kind: str, seed: int = 0):
    """The lists in another order inside every image: "reversed" (descending), "shuffled" (seeded), "sorted" (ascending)."""
    assert kind in PERMUTATIONS
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros_like(entries)
    for b, c in enumerate(counts):
        v = np.sort(entries[b, :c])
        out[b, :c] = v[::-1] if kind == "reversed" else (rng.permutation(v) if kind == "shuffled" else v)
    return out


def is_permutation_of(counts, entries, maps) -> bool:
    """Lists as read back: count[b] is the popcount of image b, its first count[b] entries a permutation of the set pixels."""
    c0, e0 = lists_of(maps)
    return bool(np.array_equal(np.asarray(counts), c0) and
                all(np.array_equal(np.sort(np.asarray(entries)[b, :c]), e0[b, :c]) for b, c in enumerate(c0)))


# ---- NaN reach --------------------------------------------------------------------------------------------------------------
def reach_formula(maps: np.ndarray, b: int, y: int, x: int) -> np.ndarray:
    """bool [B, H, W]: the candidates whose box row (and keypoint row) a NaN at input pixel (b, y, x), any channel, reaches --
    those of image b within Chebyshev distance 2: two 3 x 3 convs, then a 1 x 1."""
    B, H, W = maps.shape
    near = np.zeros((B, H, W), bool)
    near[b, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
    return maps & near


def reach_conv(maps: np.ndarray, b: int, y: int, x: int, cin: int = 2, seed: int = 0) -> np.ndarray:
    """The same set from conv_ref on a written input: a seeded finite [H, W, cin] input with one NaN, through 3x3 + SiLU,
    3x3 + SiLU and a 1x1 with seeded weights (some of them zero: a NaN times zero is NaN)."""
    B, H, W = maps.shape
    rng = np.random.Generator(np.random.PCG64(seed))
    xin = rng.standard_normal((H, W, cin))
    xin[y, x, int(rng.integers(cin))] = np.nan
    w0, w1, w2 = rng.standard_normal((3, 3, 3, cin)), rng.standard_normal((3, 3, 3, 3)), rng.standard_normal((4, 1, 1, 3))
    w0[0], w1[:, 1, 1], w2[0] = 0.0, 0.0, 0.0
    with np.errstate(all="ignore"):
        a, _ = conv_ref.conv(xin, w0, np.zeros(3), 1, 1)
        a, _ = conv_ref.conv(a, w1, np.zeros(3), 1, 1)
        a, _ = conv_ref.conv(a, w2, np.zeros(4), 1, 0)
    field = np.isnan(a)
    assert (field.all(-1) == field.any(-1)).all()          # every output channel of a reached pixel
    out = np.zeros((B, H, W), bool)
    out[b] = maps[b] & field.any(-1)
    return out
