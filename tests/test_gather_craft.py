"""tests/gather_craft.py builds what it says (CPU): every constructed candidate set has the property it is named for, on the
maps and image counts tests/test_gpu_gather_craft.py runs them at, so that nothing is vacuous on the GPU."""
import numpy as np
import pytest

import gather_craft as gc

NETS = [(64, 64), (96, 64), (224, 224)]          # (net width, net height) of the GPU module's engines
GRIDS = (1, 2, 3)
COUNTS = (1, 2, 63, 64, 65, 128, 130)


def all_dims():
    return sorted({d for w, h in NETS for d in gc.level_dims(w, h)})


def test_level_dims_and_bases():
    assert gc.level_dims(64, 64) == [(8, 8), (4, 4), (2, 2)]
    assert gc.level_dims(96, 64) == [(8, 12), (4, 6), (2, 3)]          # rows x columns
    assert gc.level_dims(224, 224) == [(28, 28), (14, 14), (7, 7)]
    assert gc.anchor_bases(gc.level_dims(96, 64)) == ([0, 96, 120], 126)


@pytest.mark.parametrize("H,W", all_dims())
def test_named_sets_have_the_property_they_are_named_for(H, W):
    s = gc.named_sets(H, W)
    assert s["empty"].sum() == 0 and s["full"].all() and s["full"].shape == (H, W)
    for name, p in (("corner_tl", (0, 0)), ("corner_tr", (0, W - 1)), ("corner_bl", (H - 1, 0)), ("corner_br", (H - 1, W - 1))):
        assert s[name].sum() == 1 and s[name][p]
    corners = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    for name, on in (("edge_top", lambda y, x: y == 0), ("edge_bottom", lambda y, x: y == H - 1),
                     ("edge_left", lambda y, x: x == 0), ("edge_right", lambda y, x: x == W - 1)):
        if name in s:
            (y, x), = np.argwhere(s[name])
            assert on(y, x) and (y, x) not in corners, name
    assert ("edge_top" in s) == (W >= 3) and ("edge_left" in s) == (H >= 3) and ("interior" in s) == (H >= 3 and W >= 3)
    if "interior" in s:
        (y, x), = np.argwhere(s["interior"])
        assert 0 < y < H - 1 and 0 < x < W - 1
        if H >= 5 and W >= 5:      # the whole 5 x 5 neighbourhood inside the map
            assert 2 <= y < H - 2 and 2 <= x < W - 2
    p, q = np.argwhere(s["neighbours"])
    assert gc.cheb(p, q) == 1      # 8-neighbours: their 5 x 5 regions overlap in 4 x 4 pixels
    c = s["checkerboard"]
    assert c[0, 0] and not (c[:, 1:] & c[:, :-1]).any() and not (c[1:] & c[:-1]).any() and c.sum() == (H * W + 1) // 2
    if H >= 2 and W >= 2:
        assert (c[1:, 1:] & c[:-1, :-1]).any()


def test_the_smallest_maps_leave_the_map_on_two_sides():
    """2 x 2 and 2 x 3 (rows x columns): every pixel's 5 x 5 neighbourhood leaves the map past at least two borders; on 4 x 4 and
    8 x 8 every pixel leaves it past at least one (every pixel a border pixel for the two 3 x 3 convs together)."""
    for H, W in ((2, 2), (2, 3)):
        assert all(gc.leaves_map_on_two_sides(H, W, y, x) for y in range(H) for x in range(W))
    assert all(gc.leaves_map_on_two_sides(4, 4, y, x) for y in range(4) for x in range(4))
    assert not gc.leaves_map_on_two_sides(28, 28, 14, 14) and gc.leaves_map_on_two_sides(28, 28, 0, 27)


def test_launch_lengths():
    n = gc.launch_lengths(GRIDS)
    assert set(gc.LENGTHS) <= set(n) and {63, 65, 127, 129, 191, 193} <= set(n)
    assert gc.passes(1) == 1 and gc.passes(32) == 1 and gc.passes(33) == 2 and gc.passes(65) == 3
    assert gc.passes_of_workgroup(65, 1) == 3                      # one workgroup, three passes: both buffer parities twice
    assert gc.passes_of_workgroup(129, 2) == 3 and gc.passes_of_workgroup(129, 2, 1) == 2
    assert gc.passes_of_workgroup(193, 3) == 3 and gc.passes_of_workgroup(191, 3) == 2
    assert gc.passes_of_workgroup(31, 3, 1) == 0                  # a workgroup without a pass


@pytest.mark.parametrize("H,W", [(28, 28), (14, 14), (7, 7)])
def test_random_launches_have_exactly_n(H, W):
    for i, n in enumerate(gc.launch_lengths(GRIDS)):
        m = gc.random_launch(100 + i, 5, H, W, n)
        assert m.shape == (5, H, W) and int(m.sum()) == n
        assert np.array_equal(m, gc.random_launch(100 + i, 5, H, W, n))
        c, _ = gc.lists_of(m)
        assert int(c.sum()) == n
        if n >= 15:
            assert (c > 0).sum() >= 2          # the list crosses an image boundary


@pytest.mark.parametrize("B", COUNTS)
@pytest.mark.parametrize("H,W", [(8, 12), (4, 6), (2, 3)])
def test_batch_layouts(B, H, W):
    lay = gc.batch_layouts(5, B, H, W)
    per = lambda m: m.reshape(B, -1).sum(1)      # noqa: E731
    assert per(lay["all_in_first"])[0] > 0 and not per(lay["all_in_first"])[1:].any()
    assert per(lay["all_in_last"])[-1] > 0 and not per(lay["all_in_last"])[:-1].any()
    for b in (63, 64):
        assert (f"only{b}" in lay) == (b < B)
        if b < B:      # image 63 is the last lane of the scan's first block, image 64 the first that needs the carry
            c = per(lay[f"only{b}"])
            assert c[b] > 0 and c.sum() == c[b]
    eo = per(lay["every_other_empty"])
    assert (eo[0::2] > 0).all() and not eo[1::2].any()
    if B >= 3:
        assert len({lay["every_other_empty"][b].tobytes() for b in range(0, B, 2)}) > 1      # different sets
    alt = per(lay["alternating"])
    assert np.array_equal(alt, np.array([(0, H * W, 1)[b % 3] for b in range(B)]))
    if B >= 12:
        ones = [tuple(np.argwhere(lay["alternating"][b])[0]) for b in range(2, B, 3)]
        assert len(set(ones)) > 1
    if B > 64:     # candidates on both sides of the 64-image block boundary in the layouts that fill the launch
        for k in ("every_other_empty", "alternating"):
            c = per(lay[k])
            assert c[:64].any() and c[64:].any()


def test_bits_round_trip_with_the_engines_anchor_bases():
    for w, h in NETS:
        dims = gc.level_dims(w, h)
        bases, A = gc.anchor_bases(dims)
        maps = {lv: gc.random_image(9 + lv, H, W, (H * W + 1) // 2) for lv, (H, W) in enumerate(dims)}
        words = gc.pack_bits(maps, dims)
        assert words.dtype == np.uint32 and len(words) == -(-A // 32)
        back = gc.unpack_bits(words, dims)
        assert all(np.array_equal(back[lv], maps[lv]) for lv in range(3))
        only = gc.pack_bits({2: gc.named_sets(*dims[2])["corner_br"]}, dims)     # the last anchor: bit A - 1, nothing past it
        assert int(only[(A - 1) // 32]) == 1 << ((A - 1) % 32) and np.count_nonzero(only) == 1
        first = gc.pack_bits({1: gc.named_sets(*dims[1])["corner_tl"]}, dims)
        assert int(first[bases[1] // 32]) == 1 << (bases[1] % 32)


def test_lists_and_permutations():
    m = gc.random_launch(3, 4, 4, 6, 33)
    c, e = gc.lists_of(m)
    assert gc.is_permutation_of(c, e, m)
    for b in range(4):
        assert np.array_equal(e[b, :c[b]], np.flatnonzero(m[b])) and not e[b, c[b]:].any()
    perms = {k: gc.permuted(c, e, k, seed=1) for k in gc.PERMUTATIONS}
    assert np.array_equal(perms["sorted"], e)
    assert not np.array_equal(perms["reversed"], e) and not np.array_equal(perms["shuffled"], e)
    assert not np.array_equal(perms["reversed"], perms["shuffled"])
    for p in perms.values():
        assert gc.is_permutation_of(c, p, m) and p.min() >= 0 and p.max() < 24
    wrong = e.copy()
    b = int(np.argmax(c))
    wrong[b, 0] = next(v for v in range(24) if v not in e[b, :c[b]])       # one entry replaced by a pixel that is no candidate
    assert not gc.is_permutation_of(c, wrong, m)
    c2 = c.copy()
    c2[0] += 1
    assert not gc.is_permutation_of(c2, e, m)


@pytest.mark.parametrize("H,W", [(28, 28), (8, 8), (4, 6), (2, 2)])
def test_nan_reach_formula_is_conv_refs(H, W):
    """Impulses at distance exactly 2 and exactly 3 from a candidate, at the border, and in another image: the formula (same
    image, Chebyshev distance <= 2) and the NaN field of conv_ref on a written input agree on the full map."""
    full = np.ones((2, H, W), bool)
    sites = [(0, 0), (H - 1, W - 1), (H // 2, W // 2), (0, W // 2)]
    for i, (y, x) in enumerate(sites):
        f, c = gc.reach_formula(full, 1, y, x), gc.reach_conv(full, 1, y, x, seed=i)
        assert np.array_equal(f, c), (y, x)
        assert not f[0].any() and f[1, y, x]
        assert int(f.sum()) == (min(y + 2, H - 1) - max(y - 2, 0) + 1) * (min(x + 2, W - 1) - max(x - 2, 0) + 1)
    if H >= 28:
        one = gc.in_image(2, H, W, 1, gc.named_sets(H, W)["interior"])
        (cy, cx), = np.argwhere(one[1])
        assert gc.reach_formula(one, 1, cy + 2, cx - 2).sum() == 1 and gc.reach_conv(one, 1, cy + 2, cx - 2).sum() == 1     # distance exactly 2
        assert gc.reach_formula(one, 1, cy + 3, cx).sum() == 0 and gc.reach_conv(one, 1, cy + 3, cx).sum() == 0         # exactly 3
        assert gc.reach_formula(one, 0, cy, cx).sum() == 0                                                                # the other image
        two = gc.in_image(1, H, W, 0, gc.named_sets(H, W)["neighbours"])
        p, q = np.argwhere(two[0])
        shared = gc.reach_formula(two, 0, p[0] + 2, p[1] + 2)                # at distance 2 of p and 1 of q
        assert shared.sum() == 2
        only_p = gc.reach_formula(two, 0, p[0] - 2, p[1] - 2)                # at distance 2 of p, 3 of q
        assert only_p.sum() == 1 and only_p[0, p[0], p[1]]
