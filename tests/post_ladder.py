"""Heads with an EXACT number of candidates, and the candidate counts worth running them at: one rung either side of every
count at which nms_pnp_kernel (csrc/k_post.hip) changes its code path.  No GPU here; tests/test_post_ladder.py checks the
builders on the CPU oracle, tests/test_gpu_post_ladder.py runs them through write_head + run_post.

The counts are computed from `capi.post_limits()` (irmv_post_limits), never written down: a pull request that moves a
threshold moves the ladder with it.  Which branch a count family is meant to reach (by the phase or helper of k_post.hip
that holds it; the constants are the ones irmv_post_limits returns):

  0, 1, 2            the empty frame (rank_sort skips its count: `if (n > 0)`), a lone key, a pair
  7, 8, 9            rank_sort's padding `n8 = (n + 7) & ~7`: seven pad keys, none, seven
  63, 64, 65         a 64-candidate block exactly full (`(n + 63) >> 6` in the walks and gather_sorted), and rank_sort's
  127, 128, 129      P = min(16, 1024 / n) lanes per key going from 16 to 15; two blocks
  pre_lo +- 1        the lower bound of the prefilter's radix window (`before >= lo` in select_window) -- reached through plateaus()
  340, 341, 342      1024 // 3: P goes from 3 to 2 (rank_sort's last stretch `j_lo < j_hi` runs empty at some n)
  rank_use +- 1      rank sort | bitonic (sort_keys), class-walk path (`kp_lds` in the kernel body), full suppression matrix
                     (`n <= kMatN`, kernel body), and the prefilter starting to run (`n_total > pre_hi`, kernel body)
  lazy_n +- 1        nms_lazy_matrix | nms_class_lists (kernel body); sixteen blocks = sixteen waves (class_word_masks)
  rank_max +- 1      the bitonic network's size 2048 -> 4096 (sort_keys) and, in attempt 0, select_window's compaction buffer
                     `pos < kRankSortMax`
  sup_cap +- 1       precomputed block masks | masks on the fly in the walk (`start < n_pre`, nms_class_lists); pre_nms_cap's default
  cand_cap +- 1      keys in LDS | exact radix select from the global list (take_keys, the kernel body's start-over, select_top_k)

Builders (each returns a complete (A, 64 + nc + nk) fp32 head with exactly n (anchor, class) pairs above the 0.25 score
threshold, every other class logit at -20):

  chain(n)           one class, neighbouring anchors, wide overlapping boxes, distinct scores: few survivors, so above
                     rank_use the prefilter's first walk neither fills max_det nor sees everything and the kernel starts
                     over (the restart rule of the attempt loop); from ~4095 up the cluster is large enough to fill 100
  iso(n)             point boxes, random pairs, random scores: nobody suppresses anybody, the first walk fills
  tied(n)            the first n pairs in (anchor, class) order at ONE logit: keys differ only in their lower 32 bits, both
                     radix searches (select_top_k, select_window) run to their last pass; several classes per anchor
  plateaus(m, n, ..) m pairs at logit 2.0, n - m at 1.0: the first radix bucket holds m keys, so the window search ends
                     above it, in it or below it as m passes pre_lo and pre_hi (select_window's wave-0 scan)
  dense(a0, a1)      every class lit on anchors [a0, a1): placed by dense_ranges() on the partition edges of both scans
                     (scan_decode_kernel's per-workgroup range, the rounds of take_keys' in-kernel scan) and on the level edges
"""
import functools

import numpy as np

NC, NK = 14, 8
DARK = np.float32(-20.0)
BLOCK = 1024                 # lanes of nms_pnp_kernel's workgroup: the rank sort's P = min(16, BLOCK // n)


def num_anchors(net):
    return sum((net // s) ** 2 for s in (8, 16, 32))


def level_edges(net):
    """First anchor of levels 1 and 2."""
    a0 = (net // 8) ** 2
    return [a0, a0 + (net // 16) ** 2]


def counts(limits):
    """The sorted candidate counts of the ladder, from irmv_post_limits' values."""
    out = {0, 1, 2, 7, 8, 9}
    for L in (64, 128, limits["pre_lo"], BLOCK // 3, limits["rank_use"], limits["lazy_n"], limits["rank_max"], limits["sup_cap"],
              limits["cand_cap"]):
        out |= {L - 1, L, L + 1}
    return sorted(out)


def scan_quads_per_block(limits, A, nc=NC):
    """scan_quads_per_block of k_post.hip: the (anchor, side) quads one scan_decode_kernel workgroup covers."""
    step, blocks = limits["scan_step"], limits["scan_blocks"]
    per = ((A * 4 + blocks - 1) // blocks + step - 1) // step * step
    cap = (limits["scan_lds_max"] // (nc * 8)) * 4 // step * step
    return min(per, cap)


@functools.lru_cache(maxsize=None)
def _base(net, boxes, nc=NC, nk=NK):
    """Everything of a head but its lit class logits (cached; builders copy it)."""
    A = num_anchors(net)
    rng = np.random.default_rng(20 + net + (boxes == "wide"))
    head = np.zeros((A, 64 + nc + nk), np.float32)
    if boxes == "wide":
        head[:, :64] = 0.05 * rng.standard_normal((A, 64))    # DFL ~ uniform: boxes of ~ +-7.5 strides around the anchor
    elif boxes == "point":
        head[:, 0:64:16] = 12.0                               # DFL mass on bin 0: zero-size boxes, no IoU exceeds anything
    else:
        raise ValueError(boxes)
    head[:, 64:64 + nc] = DARK
    head[:, 64 + nc:] = 0.25 + 0.3 * rng.standard_normal((A, nk))
    head.setflags(write=False)
    return head


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def chain(n, net=640, cls=6):
    A = num_anchors(net)
    assert 0 <= n <= A
    head = _base(net, "wide").copy()
    head[:n, 64 + cls] = np.float32(1.0) + _rng(1, n, net).permutation(n).astype(np.float32) * np.float32(1e-4)
    return head


def iso(n, net=640):
    A = num_anchors(net)
    assert 0 <= n <= A * NC
    head = _base(net, "point").copy()
    rng = _rng(2, n, net)
    pick = rng.choice(A * NC, n, replace=False)
    head[pick // NC, 64 + pick % NC] = rng.uniform(0.0, 3.0, n).astype(np.float32)
    return head


def tied(n, net=640):
    A = num_anchors(net)
    assert 0 <= n <= A * NC
    head = _base(net, "wide").copy()
    cl = np.full(A * NC, DARK, np.float32)
    cl[:n] = np.float32(1.25)
    head[:, 64:64 + NC] = cl.reshape(A, NC)
    return head


def plateaus(m, n, boxes, net=640):
    """m pairs at 2.0, the other n - m at 1.0.  The pairs are handed out from the END of the (anchor, class) order: the pair
    that joins the upper plateau when m grows by one sorts in front of every pair already on it, so the first survivor is a
    different one at every m.  "point": random pairs; "wide": one class on anchors 0 .. n - 1 (a chain: few survivors)."""
    A = num_anchors(net)
    assert 0 <= m <= n
    head = _base(net, boxes).copy()
    if boxes == "point":
        pick = np.sort(_rng(3, n, net).choice(A * NC, n, replace=False))[::-1]
    else:
        assert n <= A
        pick = (np.arange(n) * NC + 3)[::-1]
    cl = np.full(A * NC, DARK, np.float32)
    cl[pick[:m]] = np.float32(2.0)
    cl[pick[m:]] = np.float32(1.0)
    head[:, 64:64 + NC] = cl.reshape(A, NC)
    return head


def plateau_cases(limits, pre=None):
    """(m, n, boxes) around the prefilter window pre = (hi, lo), the compiled one by default."""
    hi, lo = pre or (limits["pre_hi"], limits["pre_lo"])
    ms = sorted({lo - 1, lo, lo + 1, hi - 1, hi, hi + 1})
    return [(m, n, b) for n in (hi + 1, limits["lazy_n"] + 1, limits["cand_cap"] + 1) for m in ms for b in ("point", "wide")]


def dense(a0, a1, net=640):
    A = num_anchors(net)
    assert 0 <= a0 < a1 <= A
    head = _base(net, "wide").copy()
    head[a0:a1, 64:64 + NC] = np.float32(1.25)
    return head


def dense_ranges(limits, net=640):
    """Anchor ranges on the partition edges of both scans, the level edges and the last anchor."""
    A = num_anchors(net)
    per = scan_quads_per_block(limits, A) // 4            # anchors of one scan_decode_kernel workgroup
    chunk = limits["inscan_chunk"] // 4                   # anchors of one round of the in-kernel scan
    out = [(per, min(2 * per, A)), (per - 1, per + 1), (A - 1, A)]
    out += [(e - 1, e + 1) for e in level_edges(net)]
    if chunk < (net // 8) ** 2:
        out.append((chunk - 1, chunk + 1))
    return out


def ladder(limits, net=640, builders=("chain", "iso", "tied"), max_n=None, min_n=0, with_plateaus=True, with_dense=True, pre=None):
    """[(id, builder name, args)] of a configuration; build(case) makes the head."""
    A = num_anchors(net)
    cases = []
    for n in counts(limits):
        if n < min_n or (max_n is not None and n > max_n):
            continue
        for b in builders:
            if n <= (A if b == "chain" else A * NC):
                cases.append((f"{b}({n})", b, (n,)))
    if with_plateaus:
        cases += [(f"plateaus({m}, {n}, {b})", "plateaus", (m, n, b)) for m, n, b in plateau_cases(limits, pre)]
    if with_dense:
        cases += [(f"dense({a0}, {a1})", "dense", (a0, a1)) for a0, a1 in dense_ranges(limits, net)]
    return cases


BUILDERS = dict(chain=chain, iso=iso, tied=tied, plateaus=plateaus, dense=dense)


def build(case, net=640):
    _, name, args = case
    return BUILDERS[name](*args, net=net)


def expected_count(case):
    _, name, args = case
    return (args[1] - args[0]) * NC if name == "dense" else (args[1] if name == "plateaus" else args[0])
