"""decode + NMS (csrc/k_post.hip) at every candidate count a branch switches on: the heads of tests/post_ladder.py through
write_head + run_post, each against the CPU oracle bit for bit (test_gpu_engine._assert_post_exact), one engine per test.

Which kernel branch each count family reaches is listed, with the phase or helper that holds its condition, in
tests/post_ladder.py; the configurations choose WHO gets there:

  scan            run_post as it is: scan_decode_kernel finds the candidates and decodes their boxes, nms_pnp_kernel takes the
                  keys from the global list (`if (a.counts)` in take_keys) and the rank-sort / bitonic paths of sort_keys
  keys            IRMV_POST_KEYS_ONLY=1: nms_pnp_kernel decodes its own boxes as a whole step's does -- the class-major path
                  up to rank_use candidates (`kp_lds` in the kernel body: nms_class_walk), decode_keys above
  keys-r3         ... with IRMV_NMS_CLASSWALK=0: decode_keys + the full-matrix walk at every count
  inkernel        IRMV_SPLIT_SCAN=0: the scan inside nms_pnp_kernel (take_keys' other branch), keys mirrored to the global list
                  the start-over (the kernel body's attempt loop) and the radix select (select_top_k) read back
  nopre           IRMV_NMS_PREFILTER=0: no first walk on the head of the list; every count runs the full algorithm
  pre64           IRMV_NMS_PRE=64,32: the prefilter's window moved to 32 .. 64, so its searches run at counts from 65 up and
                  the compaction / start-over logic meets the small-count paths
  wide            pre_nms_cap = cand_cap, max_det 256: survivors reach the LDS staging past record 236 (NmsLds::det_staging)
  narrow          max_det 1 with pre_nms_cap = rank_use and rank_use + 1: the first block's cap (`__popcll(K) > room`)
  cap-at-m        pre_nms_cap = m - 1, m, m + 1 around the 400 keys the first walk selects: the `n >= n_full` clause of the restart rule
  cap-at-n        pre_nms_cap = n - 1, n, n + 1 at n = rank_use, lazy_n candidates, max_det 256
  small           net 64 (84 anchors, up to 1176 pairs): several classes per anchor, one busy scan workgroup and fifteen idle
  no-anchor-list  net 1024 with IRMV_SPLIT_SCAN=0: 21 504 anchors > 4 * sup_cap, the in-kernel scan keeps no anchor list
                  (NmsLds::anchor_list returns null) and decodes every anchor's box

Beyond the oracle equality: the raw tuples of scan, keys, keys-r3, inkernel and nopre are compared with each other as the
tests run (each against the first configuration that ran in this process), pre64's against a default engine's, and after
every configuration a run_post of the empty head leaves num_dets == n_candidates == 0.

Wall time per test on the MI355X (two runs; the 640 ladder's 141 references are computed once, in the module fixture: 0.29 s
of setup): test_ladder[scan] 0.44 - 0.69 s, the other four configurations 0.15 - 0.23 s; test_pre64 0.22 - 0.40 s (two
engines); test_wide 0.12 - 0.26 s; test_narrow 0.16 - 0.21 s; test_cap_at_m 0.19 - 0.32 s and test_cap_at_n 0.20 - 0.28 s (three
engines each); test_small 0.05 - 0.11 s; test_no_anchor_list 0.49 s.  About 1.2 ms per head, upload included.

What the ladder sees that the earlier exact tests do not, tried once on a build whose restart rule read
`n + 1 >= n_full`: tied(rank_use + 1) in four configurations, iso(65) under pre64 and plateaus(400, 1025, wide) at
pre_nms_cap 401 each lose one survivor, while every exact test of test_gpu_engine.py still passes.
"""
import time

import numpy as np
import pytest

import post_ladder as pl
from irmv_detection_amd import capi
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_gpu_engine import _assert_post_exact, _raw_tuple

pytestmark = pytest.mark.gpu

SWITCHES = ("IRMV_POST_KEYS_ONLY", "IRMV_NMS_CLASSWALK", "IRMV_SPLIT_SCAN", "IRMV_EMIT_SCAN", "IRMV_NMS_PREFILTER", "IRMV_NMS_PRE")
CONFIGS = {
    "scan": {},
    "keys": dict(IRMV_POST_KEYS_ONLY="1"),
    "keys-r3": dict(IRMV_POST_KEYS_ONLY="1", IRMV_NMS_CLASSWALK="0"),
    "inkernel": dict(IRMV_SPLIT_SCAN="0"),
    "nopre": dict(IRMV_NMS_PREFILTER="0"),
}
KEYS = dict(IRMV_POST_KEYS_ONLY="1")

_REF = {}      # (case id, net, max_det, pre_nms_cap) -> the oracle's answer: computed once, shared, never modified
_RAW = {}      # configuration -> {case id: raw tuple}, as the tests of this process produced them


@pytest.fixture(scope="module")
def limits():
    oracle.build()
    return capi.post_limits()


def ref(case, net=640, md=100, cap=4096, head=None):
    key = (case[0], net, md, cap)
    if key not in _REF:
        _REF[key] = oracle.decode_nms(pl.build(case, net) if head is None else head, net, pl.NC, pl.NK, 0.25, 0.45, md, cap)
    return _REF[key]


@pytest.fixture(scope="module")
def main_ladder(limits):
    """The whole ladder of the 640 net and its references at the default caps."""
    cases = pl.ladder(limits)
    for c in cases:
        ref(c)
    return cases


def engine(monkeypatch, blob, env, cap=4096, md=100, net=640):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")            # (the conv tiles do not matter here)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return YoloEngine(None, (64, 64) if net == 64 else (1280, 1024), weights_blob=blob, net_size=net, pre_nms_cap=cap, max_det=md)


def run_cases(e, tag, cases, cap=4096, md=100, net=640):
    """Every case on engine e against the oracle; -> {case id: raw tuple}.  Ends on the empty head: nothing is carried over."""
    out = {}
    t0 = time.time()
    for case in cases:
        head = pl.build(case, net)
        try:
            raw = _assert_post_exact(e, head, max_det=md, pre_nms_cap=cap, net=net, exp=ref(case, net, md, cap, head))
            assert raw["n_candidates"] == pl.expected_count(case)
        except AssertionError as ex:
            raise AssertionError(f"configuration {tag} (pre_nms_cap {cap}, max_det {md}, net {net}), head {case[0]}: {ex}") from ex
        out[case[0]] = _raw_tuple(raw)
    e.write_head(pl.iso(0, net))
    e.run_post(0, 1)
    raw = e.read_raw(0)
    assert raw["num_dets"] == 0 and raw["n_candidates"] == 0, tag
    print(f"[post ladder] {tag} cap {cap} max_det {md} net {net}: {len(cases)} heads in {time.time() - t0:.2f} s")
    return out


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_ladder(blob, monkeypatch, main_ladder, config):
    with engine(monkeypatch, blob, CONFIGS[config]) as e:
        got = run_cases(e, config, main_ladder)
    assert len(got) == len(main_ladder) >= 130
    if _RAW:                                            # the configurations agree with each other, head by head
        other, theirs = next(iter(_RAW.items()))
        for name, t in got.items():
            assert same(t, theirs[name]), (config, other, name)
    _RAW.setdefault(config, got)


@pytest.mark.parametrize("env", [{}, KEYS], ids=["scan", "keys"])
def test_pre64(blob, monkeypatch, limits, env):
    cases = pl.ladder(limits, max_n=129, with_dense=False, pre=(64, 32))
    assert any(c[0] == "plateaus(33, 65, wide)" for c in cases) and any(c[0] == "chain(129)" for c in cases)
    with engine(monkeypatch, blob, dict(env, IRMV_NMS_PRE="64,32")) as e:
        got = run_cases(e, "pre64", cases)
    with engine(monkeypatch, blob, {}) as e:
        plain = run_cases(e, "scan (for pre64)", cases)
    for name in got:
        assert same(got[name], plain[name]), name


@pytest.mark.parametrize("env", [{}, KEYS], ids=["scan", "keys"])
def test_wide(blob, monkeypatch, limits, env):
    cap, md = limits["cand_cap"], 256
    cases = pl.ladder(limits, builders=("iso", "chain"), with_plateaus=False, with_dense=False)
    with engine(monkeypatch, blob, env, cap, md) as e:
        got = run_cases(e, "wide", cases, cap, md)
    assert got[f"iso({limits['pre_lo']})"][0] == 256          # records past 236 were staged


@pytest.mark.parametrize("over", [0, 1])
def test_narrow(blob, monkeypatch, limits, over):
    cap = limits["rank_use"] + over
    cases = pl.ladder(limits, min_n=limits["rank_use"] - 1, with_plateaus=False, with_dense=False)
    with engine(monkeypatch, blob, KEYS, cap, 1) as e:
        got = run_cases(e, "narrow", cases, cap, 1)
    assert all(t[0] == 1 for t in got.values())


@pytest.mark.parametrize("env", [{}, KEYS], ids=["scan", "keys"])
def test_cap_at_m(blob, monkeypatch, limits, env):
    m = 400
    cases = [(f"plateaus({m}, {n}, wide)", "plateaus", (m, n, "wide")) for n in (limits["pre_hi"] + 1, limits["lazy_n"] + 1, limits["cand_cap"] + 1)]
    for cap in (m - 1, m, m + 1):
        with engine(monkeypatch, blob, env, cap, 100) as e:
            got = run_cases(e, "cap-at-m", cases, cap, 100)
        assert all(1 < t[0] < 100 for t in got.values())         # the first walk did not fill max_det: only `n >= n_full` lets it stand


@pytest.mark.parametrize("which", ["rank_use", "lazy_n"])
def test_cap_at_n(blob, monkeypatch, limits, which):
    n = limits[which]
    cases = [(f"iso({n})", "iso", (n,)), (f"chain({n})", "chain", (n,))]
    for cap in (n - 1, n, n + 1):
        with engine(monkeypatch, blob, {}, cap, 256) as e:
            got = run_cases(e, "cap-at-n", cases, cap, 256)
        assert got[f"iso({n})"][0] == 256


@pytest.mark.parametrize("env", [{}, dict(IRMV_SPLIT_SCAN="0")], ids=["scan", "inkernel"])
def test_small(blob, monkeypatch, limits, env):
    cases = pl.ladder(limits, net=64, builders=("tied", "iso"), max_n=limits["lazy_n"] + 1, with_plateaus=False, with_dense=False)
    assert pl.num_anchors(64) == 84 and max(c[2][0] for c in cases) == limits["lazy_n"] + 1
    with engine(monkeypatch, blob, env, net=64) as e:
        assert e.num_anchors == 84
        run_cases(e, "small", cases, net=64)


def test_no_anchor_list(blob, monkeypatch, limits):
    net = 1024
    assert pl.num_anchors(net) > 4 * limits["sup_cap"]
    cases = [(f"{b}({n})", b, (n,)) for n in (1, limits["rank_use"], limits["rank_use"] + 1, limits["lazy_n"] + 1, limits["cand_cap"] + 1)
             for b in ("iso", "chain")]
    with engine(monkeypatch, blob, dict(IRMV_SPLIT_SCAN="0"), net=net) as e:
        assert e.num_anchors == pl.num_anchors(net)
        run_cases(e, "no-anchor-list", cases, net=net)
