"""The candidate gather (k_boxg.hip: cand_list_kernel, box_gather_kernel) alone, on WRITTEN candidates and activations.

Until here the suite reached the gather only end to end: whole steps of the one synthetic blob against an
IRMV_SPARSE_GATHER=0 / IRMV_GATHER_KPT=0 engine, at most 8 images per launch, candidate sets that are whatever the class
branch emits.  Here irmv_engine_run_op runs a level's `boxg` op on its own: the candidate bitmap is written
(irmv_engine_debug_write_cand_bits; tests/gather_craft.py), the level input is written (irmv_engine_write_tensor;
tests/act_craft.py), everything else of every tensor the launch could touch is NaN, the grid is the test's
(capi.RUN_GRID), the keypoint branch rides where a batched step links it or is left out (capi.RUN_BOX_ONLY), and the lists
may be the test's own (irmv_engine_debug_write_cand_lists + capi.RUN_WRITTEN_LISTS).

The reference of every run is the LAYER PATH on the same written state: the three box convs (and the three keypoint convs)
run in order through irmv_engine_run_conv_candidate(.., -1, ..) -- act_craft's "fused" family -- and in the same test those
layer outputs are held to conv_ref (float64) under bound() / M_REL / C_ACC / F32_UNITS exactly as
tests/test_gpu_act_craft.py holds them.  The gather is bitwise the layers at every candidate anchor (NaN masks, not payloads,
where the reference is NaN), so it is tied to float64 by two links and no tolerance is new.

Per run: the 64 box floats (and the keypoint final's 16) of every candidate anchor are the layer path's; every other head
row, every class channel, the input, the intermediates and every slot outside the range are what they were (NaN); count[level]
[image] is the popcount of the image's bits and the list a permutation of them; a level without a candidate writes nothing.

Engines (64 x 64 source frames, IRMV_AUTOTUNE=0; created once per module):

    64x3      8x8 / 4x4 / 2x2 maps: every pixel a border pixel                          sets x grids, padding
    224x5     28 / 14 / 7 maps: interiors; lists of every length of gather_craft.launch_lengths   sets x grids, list order, range, NaN reach
    96x64x130 12x8 / 6x4 / 3x2 maps, 130 slots on one stream: 1, 2, 63, 64, 65, 128, 130 images per launch, first > 0    batch
    tap224x2  act_craft.tap_blob: the ladder and +Inf
    nc1, nc16, nk0 (64 x 3), ShuffleNet int8 (224 x 3): the head row's strides, no keypoint branch

Engine creation, untuned, takes well under a second on the MI355X even at 130 slots: that engine is one
fixture of the module, used by the batch family only.

What the families cannot see: a load that is selected away, one past the allocation, and the kernels' own clamps of counts,
entries and bits out of range -- the write hooks refuse those, no test feeds them.
"""
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest

import act_craft
import class_counts
import conv_ref
import gather_craft as gc
from irmv_detection_amd import arch, capi, weights
from irmv_detection_amd.engine import YoloEngine
from test_gpu_act_craft import Case, Rig, is_poison, op_io, same_bits_and_nans, stage, touched
from test_gpu_conv_candidates import conv_ops, layer_table, run
from test_gpu_graph_ops import graph_ops, run_op

pytestmark = pytest.mark.gpu

SWITCHES = ("IRMV_GATHER_KPT", "IRMV_KPT3", "IRMV_SPARSE_GATHER", "IRMV_SPARSE_GATHER_GRID", "IRMV_FORCE_WRES", "IRMV_SPARSE_BRANCH", "IRMV_SPARSE_HEAD")
GRIDS = (1, 2, 3, 0)              # workgroups of a launch; 0: the engine's own, one per CU
BATCH_COUNTS = (1, 2, 63, 64, 65, 128, 130)
LOG = {}                          # family -> lines for DESIGN.md, printed by the last test
KPT_OFF, KPT_PAD = 80, 16         # the keypoint channels of a head record (irmv_common.hpp kKptOff; the final's cout_pad)


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ---- engines ----------------------------------------------------------------------------------------------------------
class GRig(Rig):
    """act_craft's Rig on an engine of this module: 64 x 64 source frames, untuned, every switch at its default.  (streams=1 on
    the small engines: one whose stream share is a single slot merges the first-stage Detect convs and has no boxg op.)"""

    def __init__(self, tag, blob, net_w, net_h, slots, streams=0, **pins):
        t0 = time.time()
        with env(IRMV_AUTOTUNE="0", **{**{k: None for k in SWITCHES}, **pins}):
            self.e = YoloEngine(None, (64, 64), weights_blob=blob, net_size=net_w, net_height=net_h, num_slots=slots, num_streams=streams)
        self.created = time.time() - t0
        self.tag, self.blob, self.N = tag, blob, slots
        self.share = -(-slots // self.e.num_streams)
        self.counts = [self.share, 1] if self.share > 1 else [1]
        self.ops = conv_ops(self.e)
        self.by_index = {o.op: o for o in self.ops}
        self.graph = graph_ops(self.e)
        self.table = layer_table(blob)
        self.shapes = {}
        self.dims = gc.level_dims(net_w, net_h)
        self.bases, self.A = gc.anchor_bases(self.dims)
        self.allocs = {a["name"]: i for i, a in enumerate(self.e.debug_allocs())}
        self.levels = {}

    def boxg_ops(self):
        return [g for g in self.graph if g.kind == b"boxg"]

    def level(self, lv):
        if lv not in self.levels:
            g, = [g for g in self.boxg_ops() if g.layer.decode() == f"model.22.cv2.{lv}.g"]
            self.levels[lv] = Level(self, g, lv)
        return self.levels[lv]

    # the candidate bitmap and the lists
    def write_bits(self, first, maps, lv):
        """maps bool [count, H, W] of level lv -> the bitmaps of slots [first, first + count); the other levels empty."""
        for i, m in enumerate(maps):
            w = gc.pack_bits({lv: m}, self.dims)
            capi.check(self.e._L.irmv_engine_debug_write_cand_bits(self.e._h, first + i, w.ctypes.data_as(C.POINTER(C.c_uint32)), len(w)))

    def clear_bits(self):
        w = np.zeros(-(-self.A // 32), np.uint32)
        for s in range(self.N):
            capi.check(self.e._L.irmv_engine_debug_write_cand_bits(self.e._h, s, w.ctypes.data_as(C.POINTER(C.c_uint32)), len(w)))

    def write_lists(self, lv, first, counts, entries):
        counts, entries = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(entries, np.int32)
        return self.e._L.irmv_engine_debug_write_cand_lists(self.e._h, lv, first, len(counts), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                                            entries.ctypes.data_as(C.POINTER(C.c_int32)))

    def read_lists(self, lv, first, count):
        """(counts [count], entries [count, H W]) of level lv as they lie in memory (the ranges boxg_count and boxg_list)."""
        hw = self.dims[lv][0] * self.dims[lv][1]
        c = self.e.debug_read_mem(self.allocs["boxg_count"], 4 * (lv * self.N + first), 4 * count).view(np.int32)
        l = self.e.debug_read_mem(self.allocs["boxg_list"], 4 * (self.bases[lv] * self.N + first * hw), 4 * count * hw).view(np.int32)
        return c.copy(), l.reshape(count, hw).copy()


class Level:
    """One Detect level's boxg op of a rig: what irmv_engine_op_io says of it, its layer path and its runs."""

    def __init__(self, rig, g, lv):
        self.rig, self.g, self.lv = rig, g, lv
        self.H, self.W = rig.dims[lv]
        io = op_io(rig, g.op)
        assert io.n_sub == 3 and io.n_reads == 1 and io.n_writes in (1, 2), (io.n_sub, io.n_reads, io.n_writes)
        self.subs = [rig.by_index[io.sub[i]] for i in range(3)]
        assert [o.layer.decode() for o in self.subs] == [f"model.22.cv2.{lv}.{k}" for k in range(3)]
        r = io.reads[0]
        self.read = (r.tensor.decode(), r.coff, r.C)
        self.cin = r.C
        w = [(io.writes[i].tensor.decode(), io.writes[i].coff, io.writes[i].C) for i in range(io.n_writes)]
        self.head = w[0][0]
        assert w[0] == (f"head.{lv}", 0, 64) and (self.H, self.W) == rig.shape(self.head)[:2]
        self.rides = io.n_writes == 2
        self.ksubs = []
        if self.rides:      # the level's kpt3 op reads the same segment; its sub-ops are the keypoint convs
            assert w[1] == (self.head, KPT_OFF, KPT_PAD), w[1]
            k, = [k for k in rig.graph if k.kind == b"kpt3" and k.layer.decode().startswith(f"model.22.cv4.{lv} ")]
            kio = op_io(rig, k.op)
            assert (kio.reads[0].tensor, kio.reads[0].coff, kio.reads[0].C) == (r.tensor, r.coff, r.C)
            self.ksubs = [rig.by_index[kio.sub[i]] for i in range(kio.n_sub)]
        names = {self.head, self.read[0]}
        for o in self.subs + self.ksubs:
            names |= set(touched(rig, o))
        self.names = sorted(names)
        self.top = min(act_craft.top_exponent(o.layer, rig.table[o.layer.decode()][0], False) for o in self.subs + self.ksubs)

    def range_data(self, seed, rule="postsilu"):
        return {self.read[0]: act_craft.range_bits(seed, (self.rig.N,) + self.rig.shape(self.read[0]), rule, self.top)}

    def layers(self, data, ref_slots=None, swap=None):
        """Stage `data` on every slot (NaN over everything else of every touched tensor), run the branch's conv ops in order on
        every stream share, hold each op's output to conv_ref on ref_slots -> Ref.  swap = (a, b): slot a computes from slot b's
        input (a control)."""
        rig = self.rig
        if swap:
            data = {n: v.copy() for n, v in data.items()}
            for v in data.values():
                v[swap[0]] = v[swap[1]]
        stage(rig, self.names, [self.read], data, 0, rig.N)
        ref_slots = list(range(rig.N)) if ref_slots is None else ref_slots
        worst, bad = 0.0, []
        for chain in (self.subs, self.ksubs):
            prev, src = None, data
            for o in chain:
                if not (prev is not None and prev.fused and prev.fuse_layer == o.layer):
                    for f in range(0, rig.N, rig.share):
                        c = min(rig.share, rig.N - f)
                        assert run(rig.e, o.op, 1 if c == 1 and rig.share == 1 else rig.share, -1, f, c) == capi.OK
                    case = Case(rig, o, src)
                    got = rig.read(case.out[0])
                    for s in ref_slots:
                        y, bd, _ = case.ref(s)
                        w, p = act_craft.compare(conv_ref.decode(got[s][..., case.out[1]:case.out[1] + case.out[2]], case.out[0]), y, bd, case.f32)
                        worst = max(worst, w)
                        bad += [(o.layer.decode(), s, m) for m in p]
                    src = {o.out_tensor.decode(): rig.read(o.out_tensor.decode())}
                prev = o
        before = {n: rig.read(n) for n in self.names}
        return Ref(self, data, before, worst, bad)


class Ref:
    """The layer path's state of a level: its dense head, and every touched tensor as it was when the layers were done."""

    def __init__(self, L, data, before, worst, bad):
        self.L, self.data, self.before, self.worst, self.bad = L, data, before, worst, bad
        self.head = before[L.head]
        self.nan = L.rig.nan_tensor(L.head)

    def gather(self, maps, first=0, grid=0, box_only=False, lists=None, poison_only=False, check_lists=True):
        """One run of the boxg op on slots [first, first + len(maps)) -> (problems, the head as read back).  lists =
        (counts, entries): the gather runs on them (RUN_WRITTEN_LISTS), cand_list_kernel does not run."""
        L, rig = self.L, self.L.rig
        count = len(maps)
        rig.write(L.head, self.nan)
        flags = capi.RUN_POISON | capi.RUN_GRID(grid) | (capi.RUN_BOX_ONLY if box_only else 0)
        if lists is None:
            rig.write_bits(first, maps, L.lv)
        else:
            capi.check(rig.write_lists(L.lv, first, lists[0], lists[1]))
            flags |= capi.RUN_WRITTEN_LISTS
        if poison_only:
            flags |= capi.RUN_POISON_ONLY
        run_op(rig.e, L.g.op, first, count, flags)
        got = rig.read(L.head)
        bad = []
        rows = np.zeros((rig.N, L.H, L.W), bool)
        rows[first:first + count] = maps
        keep = np.ones(got.shape, bool)
        parts = [(0, 64)] + ([(KPT_OFF, KPT_OFF + KPT_PAD)] if L.rides and not box_only else [])
        for lo, hi in parts:
            keep[rows, lo:hi] = False
            if not same_bits_and_nans([got[rows][:, lo:hi]], [self.head[rows][:, lo:hi]]):
                d = (got[rows][:, lo:hi].view(np.uint32) != self.head[rows][:, lo:hi].view(np.uint32)).any(1)
                bad.append(f"channels [{lo}, {hi}): {int(d.sum())} of {int(rows.sum())} candidate rows differ from the layer path")
        if not is_poison(got)[keep].all():
            bad.append("a head row that is no candidate's, a class channel or a slot outside the range was written")
        for n in L.names:
            if n != L.head and not np.array_equal(rig.read(n), self.before[n]):
                bad.append(f"{n}: changed by the run")
        if lists is None and check_lists and not poison_only:
            c, e = rig.read_lists(L.lv, first, count)
            if not gc.is_permutation_of(c, e, np.asarray(maps)):
                bad.append("count / list: not the popcount and a permutation of the image's bits")
            for other in range(3):
                if other != L.lv and other in [int(g.layer.decode().split(".")[3]) for g in rig.boxg_ops()]:
                    if rig.read_lists(other, first, count)[0].any():
                        bad.append(f"level {other}: a count that is not 0")
        return bad, got


@pytest.fixture(scope="module")
def rigs(blob):
    made = {}
    specs = {
        "64x3": lambda: GRig("64x3", blob, 64, 64, 3, streams=1),
        "224x5": lambda: GRig("224x5", blob, 224, 224, 5),
        "96x64x130": lambda: GRig("96x64x130", blob, 96, 64, 130, streams=1),
        "tap224x2": lambda: GRig("tap224x2", act_craft.tap_blob(blob), 224, 224, 2, streams=1),
        "nc1": lambda: GRig("nc1", class_counts.blob(1), 64, 64, 3, streams=1),
        "nc16": lambda: GRig("nc16", class_counts.blob(16), 64, 64, 3, streams=1),
        "nk0": lambda: GRig("nk0", class_counts.blob(16, 0), 64, 64, 3, streams=1),
        "shuffle-int8": lambda: GRig("shuffle-int8", weights.quantize_blob_int8(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)), 224, 224, 3, streams=1),
    }

    def get(tag):
        if tag not in made:
            made[tag] = specs[tag]()
        return made[tag]
    yield get
    for r in made.values():
        r.clear_bits() if r.boxg_ops() else None
        r.close()


def note(key, line, capsys):
    LOG.setdefault(key, []).append(line)
    with capsys.disabled():
        print("\n" + line)


def launches_of(L, B, grids_used):
    """[(name, maps [B, H, W])]: every named set on every image, and seeded launches of every length that fits the level."""
    out = [(k, np.broadcast_to(m, (B,) + m.shape).copy()) for k, m in gc.named_sets(L.H, L.W).items()]
    for i, n in enumerate(gc.launch_lengths([g for g in grids_used if g])):
        if n <= B * L.H * L.W:
            out.append((f"n{n}", gc.random_launch(1000 + 31 * L.lv + i, B, L.H, L.W, n)))
    return out


# ---- sets x grids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_only", [False, True], ids=["kpt", "box"])
@pytest.mark.parametrize("lv", [0, 1, 2])
@pytest.mark.parametrize("tag", ["224x5", "64x3"])
def test_sets_and_grids(rigs, capsys, tag, lv, box_only):
    rig, t0 = rigs(tag), time.time()
    L = rig.level(lv)
    assert L.rides and L.cin == (64, 128, 256)[lv]
    ref = L.layers(L.range_data(11 + lv))
    assert not ref.bad, ref.bad[:5]
    bad, runs, most = [], 0, 0
    for name, maps in launches_of(L, rig.N, GRIDS):
        n = int(maps.sum())
        for grid in GRIDS:
            p, got = ref.gather(maps, 0, grid, box_only)
            bad += [(name, grid, m) for m in p]
            runs += 1
            if grid == 1:
                most = max(most, gc.passes_of_workgroup(n, 1))
        if n == 0:
            assert is_poison(got).all()          # a level without a candidate writes nothing
    # one workgroup walked every pass of the full map: at least three wherever the level has 65 anchors in the launch
    assert most == gc.passes(rig.N * L.H * L.W) and (most >= 3 or rig.N * L.H * L.W < 65), most
    if tag == "224x5":
        assert most >= 3
    note("sets", f"[gather craft {tag} level {lv} {'box' if box_only else 'box + kpt'}] {runs} runs, most passes of one workgroup {most}, "
         f"layer path worst err/bound {ref.worst:.3f}; {time.time() - t0:.1f} s", capsys)
    assert not bad, bad[:10]


# ---- batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [0, 1, 2])
def test_batch_layouts_and_image_counts(rigs, capsys, lv):
    """130 slots on one stream.  The layer path runs once on all of them (every image its own input: an image resolved to the
    wrong prefix reads another image's pixels and cannot match); the gather runs on 1 .. 130 images, from slot 0 and from
    first > 0, every layout of gather_craft.batch_layouts."""
    rig, t0 = rigs("96x64x130"), time.time()
    L = rig.level(lv)
    ref = L.layers(L.range_data(40 + lv), ref_slots=[0, 1, 63, 64, 65, 129])
    assert not ref.bad, ref.bad[:5]
    bad, runs = [], 0
    for B in BATCH_COUNTS:
        firsts = [0] + ([rig.N - B] if 0 < rig.N - B else []) + ([65] if B == 65 else [])
        for first in dict.fromkeys(firsts):
            for name, maps in gc.batch_layouts(7 * B + first + lv, B, L.H, L.W).items():
                for grid, box_only in ((0, False), (2, B in (65, 130))):
                    p, _ = ref.gather(maps, first, grid, box_only)
                    bad += [(B, first, name, grid, m) for m in p]
                    runs += 1
    note("batch", f"[gather craft 96x64x130 level {lv}] {runs} runs at image counts {BATCH_COUNTS}, layer path worst err/bound {ref.worst:.3f}; "
         f"engine created in {rig.created:.1f} s; {time.time() - t0:.1f} s", capsys)
    assert not bad, bad[:10]


# ---- list order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [0, 1, 2])
def test_no_stored_bit_depends_on_the_lists_order(rigs, lv):
    rig = rigs("224x5")
    L = rig.level(lv)
    ref = L.layers(L.range_data(70 + lv))
    for k, maps in enumerate([gc.random_launch(5, rig.N, L.H, L.W, 65), gc.random_launch(6, rig.N, L.H, L.W, 193),
                              np.broadcast_to(gc.named_sets(L.H, L.W)["checkerboard"], (rig.N, L.H, L.W)).copy()]):
        p, own = ref.gather(maps, 0, 2)
        assert not p, p
        counts, entries = rig.read_lists(lv, 0, rig.N)
        for kind in gc.PERMUTATIONS:
            lists = (counts, gc.permuted(counts, entries, kind, seed=k))
            for grid in (1, 0):
                p, got = ref.gather(maps, 0, grid, lists=lists)
                assert not p, (kind, grid, p)
                assert same_bits_and_nans([got], [own]), (kind, grid)


# ---- range and ladder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [0, 1, 2])
def test_range_signed_and_inf(rigs, capsys, lv):
    """act_craft's "signed" magnitudes (the "postsilu" ones are every other family's input), then +Inf at seeded input
    elements: the layer path gives Inf and NaN rows, and the gather the same masks."""
    rig = rigs("224x5")
    L = rig.level(lv)
    maps = np.broadcast_to(gc.named_sets(L.H, L.W)["full"], (rig.N, L.H, L.W)).copy()
    data = L.range_data(90 + lv, "signed")
    ref = L.layers(data)
    assert not ref.bad, ref.bad[:5]
    worst = ref.worst
    for grid in (0, 3):
        p, _ = ref.gather(maps, 0, grid)
        assert not p, p
    rng = np.random.Generator(np.random.PCG64(lv))
    t = data[L.read[0]]
    for s in range(rig.N):
        for _ in range(3):
            t[s, int(rng.integers(L.H)), int(rng.integers(L.W)), L.read[1] + int(rng.integers(L.cin))] = 0x7C00
    ref = L.layers(data)
    assert not ref.bad, ref.bad[:5]
    assert not np.isfinite(ref.head[..., :64]).all()
    for grid in (0, 3):
        p, _ = ref.gather(maps, 0, grid)
        assert not p, p
    note("range", f"[gather craft 224x5 level {lv} signed, +Inf] layer path worst err/bound {max(worst, ref.worst):.3f}", capsys)


@pytest.mark.parametrize("lv", [0, 1, 2])
def test_ladder_on_the_tap_blob(rigs, capsys, lv):
    """Every exponent of fp16, both signs, +-0, subnormals, the largest values and +Inf as pre-activations of the first conv."""
    rig = rigs("tap224x2")
    L = rig.level(lv)
    name = L.read[0]
    maps = np.broadcast_to(gc.named_sets(L.H, L.W)["full"], (rig.N, L.H, L.W)).copy()
    assert act_craft.ladder_parts((rig.N,) + rig.shape(name)) <= 2
    worst = 0.0
    for part in range(act_craft.ladder_parts((rig.N,) + rig.shape(name))):
        ref = L.layers({name: act_craft.tile_ladder((rig.N,) + rig.shape(name), part)})
        assert not ref.bad, ref.bad[:5]
        worst = max(worst, ref.worst)
        for grid in (0, 1):
            p, _ = ref.gather(maps, 0, grid)
            assert not p, p
    note("range", f"[gather craft tap224x2 level {lv} ladder] layer path worst err/bound {worst:.3f}", capsys)


# ---- NaN reach ----------------------------------------------------------------------------------------------------------------
def _impulse_cases(L):
    """[(name, candidate pixel, impulse (dslot, y, x, channel of the tensor), reaches)] around one candidate of slot 1."""
    H, W, (name, coff, Cc) = L.H, L.W, L.read
    cy, cx = H // 2, W // 2
    Ct = L.rig.shape(name)[2]
    cases = [("distance 2", (cy, cx), (0, cy + 2, cx - 2, coff), True), ("distance 3", (cy, cx), (0, cy + 3, cx, coff), False),
             ("distance 3 in x", (cy, cx), (0, cy, cx - 3, coff + Cc - 1), False),
             ("last channel of the segment", (cy, cx), (0, cy - 1, cx + 2, coff + Cc - 1), True),
             ("corner candidate, distance 2", (0, 0), (0, 2, 2, coff + 1), True), ("corner candidate, distance 3", (0, 0), (0, 3, 0, coff), False),
             # across the border: row-wrapped neighbours of a candidate in the first column / the last row
             ("wrapped: the last pixel of the row above", (cy, 0), (0, cy - 1, W - 1, coff), False),
             ("wrapped: the first row under the last", (H - 1, cx), (0, 0, cx, coff), False),
             ("the next slot, same pixel", (cy, cx), (1, cy, cx, coff), False), ("the slot before, same pixel", (cy, cx), (-1, cy, cx, coff), False)]
    if coff + Cc < Ct:
        cases.append(("the channel behind the segment", (cy, cx), (0, cy, cx, coff + Cc), False))
    if coff > 0:
        cases.append(("the channel in front of the segment", (cy, cx), (0, cy, cx, coff - 1), False))
    return cases


@pytest.mark.parametrize("lv", [0, 1, 2])
def test_nan_reach(rigs, capsys, lv):
    """One candidate in slot 1 of 3 written slots, impulses one at a time in a finite input (the undeclared channels and slots
    are NaN in every run of this module anyway): isnan(out) is exactly the reference's set -- conv_ref's through the layer
    path, and gather_craft.reach_formula's."""
    rig = rigs("224x5")
    L = rig.level(lv)
    name = L.read[0]
    clean = L.range_data(120 + lv)
    reached = 0
    for what, (cy, cx), (ds, y, x, ch), reaches in _impulse_cases(L):
        data = {name: clean[name].copy()}
        data[name][1 + ds, y, x, ch] = act_craft.NAN_BITS
        maps = np.zeros((3, L.H, L.W), bool)
        maps[1, cy, cx] = True
        inside = L.read[1] <= ch < L.read[1] + L.read[2]
        want = gc.reach_formula(maps, 1 + ds, y, x) if inside else np.zeros_like(maps)
        assert bool(want.any()) == reaches, what
        ref = L.layers(data, ref_slots=[1, 1 + ds])
        assert not ref.bad, (what, ref.bad[:5])          # (compare() holds the layers' NaN set to conv_ref's)
        layer_nan = np.isnan(ref.head[:3][..., :64]).all(-1) & maps
        assert np.array_equal(layer_nan, want), what
        for box_only in (False, True):
            p, got = ref.gather(maps, 0, 0, box_only)
            assert not p, (what, p)
            row = got[1, cy, cx]
            assert np.isnan(row[:64]).all() == reaches and np.isnan(row[:64]).any() == reaches, what
            if not box_only:
                assert np.isnan(row[KPT_OFF:KPT_OFF + 8]).all() == reaches, what
        reached += int(want.sum())
    assert reached >= 3
    # a full map around one impulse: exactly the 5 x 5 neighbourhood of the same image
    data = {name: clean[name].copy()}
    data[name][2, 1, L.W - 2, L.read[1] + 3] = act_craft.NAN_BITS
    maps = np.ones((rig.N, L.H, L.W), bool)
    ref = L.layers(data, ref_slots=[2])
    assert not ref.bad, ref.bad[:5]
    p, got = ref.gather(maps, 0, 2)
    assert not p, p
    assert np.array_equal(np.isnan(got[..., :64]).any(-1), gc.reach_formula(maps, 2, 1, L.W - 2))
    assert np.array_equal(np.isnan(got[..., KPT_OFF:KPT_OFF + 8]).any(-1), gc.reach_formula(maps, 2, 1, L.W - 2))


# ---- padding ----------------------------------------------------------------------------------------------------------------
def _biased(blob, value):
    hdr, layers = weights.parse_blob(blob)
    specs, tensors = [], []
    for sp, w, b in layers:
        b = b.copy()
        if sp.name.startswith("model.22.cv2.") and sp.name.endswith(".0"):
            b[:] = value
        specs.append(sp)
        tensors.append((w.copy(), b))
    return weights.build_blob(specs, tensors, hdr["nc"], hdr["nk"], hdr["backbone"])


@pytest.mark.parametrize("net_w,net_h", [(64, 64), (96, 64)])
def test_padding_is_zero_not_silu_of_the_bias(blob, capsys, net_w, net_h):
    """The box branch's first-conv bias at 4.07 on every channel: SiLU(bias) = 4.0.  A position outside the map is the second
    conv's zero padding; a kernel that computes the first conv there (zero inputs: SiLU(bias)) and does not zero it is off by
    4 * sum of the second conv's border taps.  Full maps: the corners of the 2 x 2 and 3 x 2 maps are bitwise the layers'."""
    rig = GRig("pad", _biased(blob, 4.07), net_w, net_h, 3, streams=1)
    try:
        for lv in range(3):
            L = rig.level(lv)
            ref = L.layers(L.range_data(200 + lv))
            assert not ref.bad, ref.bad[:5]
            z = np.zeros((1,) + rig.shape(L.read[0]), np.uint16)      # what padding WOULD give if it were computed: the first conv of a zero input
            mid = Case(rig, L.subs[0], {L.read[0]: np.repeat(z, rig.N, 0)}).ref(0)[0]
            assert np.allclose(mid, 4.0, atol=0.01)
            maps = np.ones((rig.N, L.H, L.W), bool)
            for grid in (1, 0):
                p, _ = ref.gather(maps, 0, grid)
                assert not p, (lv, grid, p)
        rig.clear_bits()
    finally:
        rig.close()


# ---- other head strides, no keypoint branch, the other backbone ---------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nc1", "nc16", "nk0", "shuffle-int8"])
def test_other_models(rigs, capsys, tag):
    rig = rigs(tag)
    has = sorted(g.layer.decode() for g in rig.boxg_ops())
    note("models", f"[gather craft {tag}] boxg ops: {has}; engine created in {rig.created:.1f} s", capsys)
    if tag == "shuffle-int8" and not has:
        return                       # (asserted from irmv_engine_ops: this model's box branches are no gather's)
    assert has == [f"model.22.cv2.{lv}.g" for lv in range(3)], has
    for lv in range(3):
        L = rig.level(lv)
        assert L.rides == (tag != "nk0")
        ref = L.layers(L.range_data(300 + lv))
        assert not ref.bad, ref.bad[:5]
        for name, maps in launches_of(L, rig.N, (1,)):
            for grid in (1, 0):
                p, _ = ref.gather(maps, 0, grid)
                assert not p, (tag, lv, name, grid, p)


# ---- the hooks themselves -------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_the_kernels_would_clamp(rigs):
    rig = rigs("64x3")
    e, L_ = rig.e, rig.e._L
    nw = -(-rig.A // 32)
    w = np.zeros(nw + 1, np.uint32)
    p = w.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L_.irmv_engine_debug_write_cand_bits(e._h, 0, p, nw + 1) == capi.ERR_ARG
    assert L_.irmv_engine_debug_write_cand_bits(e._h, 0, p, nw - 1) == capi.ERR_ARG
    assert L_.irmv_engine_debug_write_cand_bits(e._h, rig.N, p, nw) == capi.ERR_ARG
    assert rig.A % 32 != 0                                   # 84 anchors: the last word has 12 bits past the last anchor
    w[nw - 1] = 1 << (rig.A % 32)
    assert L_.irmv_engine_debug_write_cand_bits(e._h, 0, p, nw) == capi.ERR_ARG
    w[nw - 1] = 1 << (rig.A % 32 - 1)
    capi.check(L_.irmv_engine_debug_write_cand_bits(e._h, 0, p, nw))
    assert np.array_equal(e.debug_cand_bits(0)[1], w[:nw])
    w[:] = 0
    capi.check(L_.irmv_engine_debug_write_cand_bits(e._h, 0, p, nw))
    H, W = rig.dims[1]
    ok_c, ok_e = np.array([H * W, 0], np.int32), np.zeros((2, H * W), np.int32)
    ok_e[0] = np.arange(H * W)
    assert rig.write_lists(1, 1, ok_c, ok_e) == capi.OK
    c, l = rig.read_lists(1, 1, 2)
    assert np.array_equal(c, ok_c) and np.array_equal(l, ok_e)
    for c_bad in ([H * W + 1, 0], [-1, 0]):
        assert rig.write_lists(1, 1, np.array(c_bad, np.int32), ok_e) == capi.ERR_ARG
    for v in (H * W, -1):
        e_bad = ok_e.copy()
        e_bad[1, 3] = v
        assert rig.write_lists(1, 1, ok_c, e_bad) == capi.ERR_ARG
    assert rig.write_lists(3, 0, ok_c, ok_e) == capi.ERR_ARG and rig.write_lists(1, 2, ok_c, ok_e) == capi.ERR_ARG
    g = rig.boxg_ops()[0]
    assert L_.irmv_engine_run_op(e._h, g.op, 0, rig.N + 1, 0) == capi.ERR_ARG
    assert L_.irmv_engine_run_op(e._h, g.op, 0, 1, 16) == capi.ERR_ARG                      # an unknown flag bit
    pool, = [o for o in rig.graph if o.kind == b"pool"]
    assert L_.irmv_engine_run_op(e._h, pool.op, 0, 1, capi.RUN_BOX_ONLY) == capi.ERR_ARG      # a boxg flag on another op


def test_no_engine_has_more_slots_than_a_launch_holds(blob):
    """box_gather_kernel holds the prefix of at most 1024 images (GMAXB), and fuse_boxg gives an engine of more slots no boxg op.
    No such engine exists: irmv_engine_create refuses more than 256 slots, so the guard cannot be shown on a plan -- what is
    shown is that creation refuses.  Nothing runs."""
    for slots in (257, 1025):
        with pytest.raises(capi.IrmvError) as ei:
            GRig("too many", blob, 64, 64, slots, streams=1)
        assert ei.value.code == capi.ERR_ARG and "num_slots" in str(ei.value)


def test_an_engine_without_a_sparse_head_refuses(blob):
    """IRMV_SPARSE_HEAD=0: the write hook and the op's run are refused."""
    rig = GRig("dense", blob, 64, 64, 2, streams=1, IRMV_SPARSE_HEAD="0")
    try:
        w = np.zeros(-(-rig.A // 32), np.uint32)
        assert rig.e._L.irmv_engine_debug_write_cand_bits(rig.e._h, 0, w.ctypes.data_as(C.POINTER(C.c_uint32)), len(w)) == capi.ERR_ARG
        for g in rig.boxg_ops():
            assert rig.e._L.irmv_engine_run_op(rig.e._h, g.op, 0, 1, 0) == capi.ERR_ARG
    finally:
        rig.close()


# ---- controls -------------------------------------------------------------------------------------------------------------------
def test_controls(rigs):
    """Each check fails when it must: a poison-only run fails the comparison with the layers; a list with one entry replaced by
    its neighbour fails the rows check; a layer path that ran slot 1 on slot 2's input fails bitwise."""
    rig = rigs("224x5")
    L = rig.level(1)
    data = L.range_data(400)
    ref = L.layers(data)
    maps = gc.random_launch(8, rig.N, L.H, L.W, 33)
    p, own = ref.gather(maps, 0, 2)
    assert not p, p
    p, _ = ref.gather(maps, 0, 2, poison_only=True)
    assert any("differ from the layer path" in m for m in p), p
    counts, entries = rig.read_lists(1, 0, rig.N)
    b = int(np.argmax(counts))
    moved = entries.copy()
    taken = set(entries[b, :counts[b]].tolist())
    moved[b, 0] = next(v for v in (entries[b, 0] + 1, entries[b, 0] - 1, entries[b, 0] + L.W) if 0 <= v < L.H * L.W and v not in taken)
    p, _ = ref.gather(maps, 0, 2, lists=(counts, moved))
    assert any("differ from the layer path" in m for m in p) and any("no candidate's" in m for m in p), p
    assert not gc.is_permutation_of(counts, moved, maps)
    wrong = L.layers(data, swap=(1, 2))
    full = np.ones((rig.N, L.H, L.W), bool)
    p, _ = wrong.gather(full, 0, 0)
    assert not p, p                                  # (consistent with itself ...)
    assert not same_bits_and_nans([wrong.head[1]], [ref.head[1]]) and same_bits_and_nans([wrong.head[1]], [ref.head[2]])
    assert same_bits_and_nans([wrong.head[0]], [ref.head[0]])
    p, _ = ref.gather(full, 0, 0)                    # (... and not with the layers that ran every slot on its own input)
    assert any(f"{L.H * L.W} of {rig.N * L.H * L.W} candidate rows differ from the layer path" in m for m in p), p


# ---- slow -----------------------------------------------------------------------------------------------------------------------
def test_slow_256_slot_launch(blob, capsys):
    """256 images in one launch, the most an engine can have (the kernel's GMAXB of 1024 is out of any engine's reach): four
    blocks of the prefix scan, three carries."""
    rig = GRig("64x256", blob, 64, 64, 256, streams=1)
    try:
        for lv in (0, 2):
            L = rig.level(lv)
            ref = L.layers(L.range_data(500 + lv), ref_slots=[0, 63, 64, 127, 128, 192, 255])
            assert not ref.bad, ref.bad[:5]
            lay = gc.batch_layouts(3, 256, L.H, L.W)
            for b in (127, 128, 191, 192, 255):
                lay[f"only{b}"] = gc.in_image(256, L.H, L.W, b, gc.random_image(b, L.H, L.W, L.H * L.W // 3 + 1))
            for name, maps in lay.items():
                for grid in (0, 1):
                    p, _ = ref.gather(maps, 0, grid)
                    assert not p, (lv, name, grid, p)
        note("slow", f"[gather craft 64x256] engine created in {rig.created:.1f} s", capsys)
        rig.clear_bits()
    finally:
        rig.close()


def test_zz_log(capsys):
    """The lines of DESIGN.md section 33, as this run measured them."""
    with capsys.disabled():
        for key in sorted(LOG):
            print("\n".join(LOG[key]))
