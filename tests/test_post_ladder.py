"""The ladder's builders (tests/post_ladder.py) on the CPU oracle: every head carries exactly the candidates it claims, and
the properties the GPU ladder leans on hold -- chain() leaves the prefilter's first walk short of max_det, iso() fills it,
plateaus() shows a threshold that is off by one.  No GPU; oracle.decode_nms costs ~ 20 ms per 640 head."""
import functools
import os
import re

import pytest

import post_ladder as pl
from conftest import ROOT
from irmv_detection_amd import _build, capi
from oracle import oracle


@pytest.fixture(scope="module")
def limits():
    _build.build()
    oracle.build()
    return capi.post_limits()


@functools.lru_cache(maxsize=None)
def ref(case, net=640, max_det=100, pre_nms_cap=4096):
    """The oracle's answer for a ladder case: computed once, shared, never modified."""
    return oracle.decode_nms(pl.build(case, net), net, pl.NC, pl.NK, 0.25, 0.45, max_det, pre_nms_cap)


def survivors(r):
    return list(zip(r["anchors"].tolist(), r["classes"].tolist()))


def test_limits_are_the_kernels_constants(limits):
    """irmv_post_limits against what k_post.hip and irmv_common.hpp spell out, and against the header's own bounds."""
    src = open(os.path.join(ROOT, "irmv_detection_amd", "csrc", "k_post.hip")).read()
    named = dict(rank_use="kRankSortUse", rank_max="kRankSortMax", lazy_n="kLazyN_", sup_cap="kSupCap")
    for key, name in named.items():
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == limits[key], key
    hi, lo = re.search(r"constexpr int kPreHi = (\d+), kPreLo = (\d+);", src).groups()
    assert (int(hi), int(lo)) == (limits["pre_hi"], limits["pre_lo"])
    assert limits["cand_cap"] == capi.CAND_CAP
    assert limits["mat_n"] == limits["rank_use"] == limits["pre_hi"]         # three names of one count in the kernel
    assert limits["pre_lo"] < limits["pre_hi"] <= limits["lazy_n"] <= limits["rank_max"] <= limits["sup_cap"] <= limits["cand_cap"]
    assert limits["max_tiles"] == 16 and limits["max_det_cap"] == 256         # IRMV_MAX_TILES, IRMV_MAX_DET_CAP


def test_counts_follow_the_limits(limits):
    c = pl.counts(limits)
    assert c == sorted(set(c)) and c[:6] == [0, 1, 2, 7, 8, 9]
    for key in ("pre_lo", "rank_use", "lazy_n", "rank_max", "sup_cap", "cand_cap"):
        assert {limits[key] - 1, limits[key], limits[key] + 1} <= set(c), key
    assert {63, 64, 65, 127, 128, 129, 340, 341, 342} <= set(c)
    # a threshold that moves takes its rungs along
    moved = dict(limits, rank_use=640, lazy_n=1536, pre_lo=300)
    m = pl.counts(moved)
    assert {639, 640, 641, 1535, 1536, 1537, 299, 300, 301} <= set(m)
    for gone in (limits["rank_use"], limits["lazy_n"], limits["pre_lo"]):
        assert gone not in m or gone in {64, 128, pl.BLOCK // 3}
    assert [m_ for m_, _, _ in pl.plateau_cases(moved)[:12:2]] == [299, 300, 301, 511, 512, 513]
    assert pl.plateau_cases(limits, pre=(64, 32))[0] == (31, 65, "point")
    # the scan's partition (640 anchors per scan_decode_kernel workgroup on the 640 net) follows irmv_post_limits too
    assert pl.scan_quads_per_block(limits, 8400) == 2560 * (limits["scan_step"] // 512) or limits["scan_step"] != 512
    assert pl.scan_quads_per_block(dict(limits, scan_blocks=8), 8400) > pl.scan_quads_per_block(limits, 8400)


def test_every_head_has_exactly_its_candidates(limits):
    for case in pl.ladder(limits):
        assert ref(case)["n_candidates"] == pl.expected_count(case), case[0]
    for case in pl.ladder(limits, pre=(64, 32), builders=(), with_dense=False):
        assert ref(case)["n_candidates"] == pl.expected_count(case), case[0]


def test_small_and_large_net_heads(limits):
    small = pl.ladder(limits, net=64, builders=("tied", "iso"), max_n=limits["lazy_n"] + 1, with_plateaus=False, with_dense=False)
    assert len(small) == 2 * sum(n <= limits["lazy_n"] + 1 for n in pl.counts(limits))     # 84 x 14 = 1176 pairs hold them all
    for case in small:
        assert ref(case, 64)["n_candidates"] == case[2][0], case[0]
    assert pl.num_anchors(1024) > 4 * limits["sup_cap"]                     # the kernel's anchor list does not exist
    for n in (1, limits["rank_use"] + 1, limits["cand_cap"] + 1):
        for b in ("iso", "chain"):
            assert ref((f"{b}({n})", b, (n,)), 1024)["n_candidates"] == n


def test_chain_leaves_the_first_walk_short(limits):
    """Above rank_use the prefilter's first walk sees the best <= pre_hi of a chain: it must neither fill max_det nor be the
    whole list, or the start-over (`s_kept >= max_det || n >= n_full`) is not reached."""
    for n in pl.counts(limits):
        if limits["rank_use"] < n <= limits["rank_max"] + 1:
            r = ref((f"chain({n})", "chain", (n,)))
            assert 1 < r["num_dets"] < 100, (n, r["num_dets"])
            # ... and the best pre_hi alone keep fewer still (the walk the kernel takes first)
            head = pl.chain(n)
            first = oracle.decode_nms(head, 640, pl.NC, pl.NK, 0.25, 0.45, 100, limits["pre_hi"])
            assert first["num_dets"] < 100 and limits["pre_hi"] < n
    top = max(n for n in pl.counts(limits) if n <= pl.num_anchors(640))
    assert ref((f"chain({top})", "chain", (top,)))["num_dets"] == 100      # the largest chain fills max_det


def test_iso_fills(limits):
    for n in pl.counts(limits):
        r = ref((f"iso({n})", "iso", (n,)))
        assert r["num_dets"] == min(n, 100), n
    n = limits["rank_use"]
    assert ref((f"iso({n})", "iso", (n,)), 640, 256, n - 1)["num_dets"] == 256      # cap-at-n: pre_nms_cap and max_det bind


def test_tied_order_is_anchor_then_class(limits):
    r = ref(("tied(129)", "tied", (129,)))
    s = survivors(r)
    assert s == sorted(s) and len(set(r["scores"].tolist())) == 1 and s[0] == (0, 0)
    assert len({a for a, _ in s}) < len(s)                                # several classes of one anchor survive side by side


@pytest.mark.parametrize("pre", [None, (64, 32)])
def test_plateaus_show_an_off_by_one(limits, pre):
    """The survivor list at m and at m + 1 differs (in its first entry): a window search that ends one key early or late
    cannot return the same list by accident."""
    cases = pl.plateau_cases(limits, pre)
    assert len(cases) == 36
    for m, n, boxes in cases:
        m = min(m, n - 1)                                                  # (m = n: every pair on the upper plateau; its neighbour is m - 1)
        a = ref((f"plateaus({m}, {n}, {boxes})", "plateaus", (m, n, boxes)))
        b = ref((f"plateaus({m + 1}, {n}, {boxes})", "plateaus", (m + 1, n, boxes)))
        assert a["n_candidates"] == b["n_candidates"] == n
        assert survivors(a) != survivors(b) and survivors(a)[0] != survivors(b)[0], (m, n, boxes)


def test_cap_at_m_reaches_the_restart_rule(limits):
    """plateaus(400, n, "wide") under pre_nms_cap 399 / 400 / 401: the first walk sees the 400 keys of the upper plateau, keeps
    fewer than max_det of them, and the three caps give three different answers to `n >= n_full`."""
    m = 400
    assert limits["pre_lo"] <= m <= limits["pre_hi"]
    for n in (limits["pre_hi"] + 1, limits["lazy_n"] + 1, limits["cand_cap"] + 1):
        case = (f"plateaus({m}, {n}, wide)", "plateaus", (m, n, "wide"))
        got = [ref(case, 640, 100, cap) for cap in (m - 1, m, m + 1)]
        assert all(1 < g["num_dets"] < 100 for g in got), [g["num_dets"] for g in got]
        assert all(g["n_candidates"] == n for g in got)


def test_dense_ranges_sit_on_the_partitions(limits):
    r = pl.dense_ranges(limits)
    per = pl.scan_quads_per_block(limits, 8400) // 4
    assert (per, 2 * per) in r and (per - 1, per + 1) in r and (8399, 8400) in r
    assert (6399, 6401) in r and (7999, 8001) in r
    assert (limits["inscan_chunk"] // 4 - 1, limits["inscan_chunk"] // 4 + 1) in r
    assert per * pl.NC > limits["cand_cap"]                                # one workgroup alone overflows the LDS key list
