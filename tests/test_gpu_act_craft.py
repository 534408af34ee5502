"""Every conv op, every tile candidate and every fused kernel on WRITTEN activations (tests/act_craft.py).

The conv sweep (tests/test_gpu_conv_candidates.py), the op checks (tests/test_gpu_graph_ops.py) and the "fused kernel is
bitwise its layers" comparisons all take a kernel's input from the engine's own forward pass: synthetic frames through the one
variance-calibrated synthetic blob, activations in [-0.279, 18.5].  Here irmv_engine_write_tensor puts chosen values in
front of each kernel, run on its own through irmv_engine_run_conv_candidate / irmv_engine_run_op:

    range     (a) magnitudes from the smallest subnormal to ~4000 (lower where a layer's outputs would leave fp16:
              act_craft.top_exponent), as a SiLU leaves them ("postsilu") and with both signs ("signed").  The engine's own
              choice on every slot range of ranges_for() is inside the bound() of the conv sweep (M_REL, C_ACC unchanged)
              against conv_ref on the written inputs, and finite; every listed candidate, on (0, share) or (N - 1, 1), is
              bitwise the own choice.
    ladder    (b) on an engine of act_craft.tap_blob, where a pre-activation IS an input value: every exponent of fp16, both
              signs, +-0, subnormals, the largest values and +Inf through every activated conv op and every candidate, under
              the same bound -- here the fp16 rounding, 4 * 2^-24 |x| and the subnormal floor.  +Inf in gives +Inf out; candidates
              are bitwise the own choice outside the NaNs (a NaN's sign and payload are each kernel's own).
    NaN reach (c) NaN impulses in a finite input: isnan(out) is isnan(reference) exactly, every other element bitwise the
              impulse-free run's.
    fused     (d) c2f2, c2f32, bneck and kpt3 on the inputs of (a) and (c) give, on every range irmv_engine_op_io says they
              write, the bits their conv ops leave when run in order from the same written inputs; equal NaN masks.

Every run writes the declared inputs and NaN (all-ones) over EVERYTHING ELSE of every activation tensor the op touches: the
other channels, every slot outside [first, first + count), the output.  A load of anything undeclared -- a neighbouring slot,
another channel range of a concat tensor, the row-wrapped neighbour of a border pixel -- that is multiplied by a zero weight or
masked by arithmetic instead of a select then turns an output into NaN; after the run everything the run was not to write is
still NaN.  Controls show that the checks fail when they must.

Finding: the fp32 Detect finals (1x1, bias only, fp32 out: model.22.cv{2,3,4}.N.2 run as their own launches) exceed
C_ACC = 4 on `range` inputs: worst err / bound 1.172 (model.22.cv2.0.2, 224 x 5, "postsilu"; 1.107 "signed"; the keypoint
finals 1.036; 0.96 on 224 x 1 and 64 x 3, which have fewer samples), i.e. 4.7 units of 2^-24 (|b| + sum |w||x|).  The kernel
is not wrong: the count "one fp32 rounding per MFMA" behind C_ACC does not hold.  v_mfma_f32_16x16x32_f16 adds its 32 products
to the accumulator in four groups of eight (v_mfma_f32_16x16x16_f16: two groups), each group with one round-to-nearest of the
accumulator; inside a group the products are aligned to the group's largest one and the bits below its last place are dropped,
and against a larger accumulator they keep at least five more bits.  (Measured on the MI355X with crafted operands, scripts/mfma_rounding_probe.cpp: C = 2^24
and 32 products of 3/4, 3/8, 3/16, 3/32 give 2^24 + 24, + 16, + 8, + 0, where one rounding at the end would give + 24, + 12,
+ 6, + 4; C = 0, one product 2^24 and 31 of 3/4 give 2^24 + 18, the seven products beside the large one lost.)  Counted for
a final with K input channels, in units of 2^-24 (|b| + sum |w||x|):

    K / 8   accumulator roundings, one per group (<= 2^-24 |partial sum| each)
    K / 16  products aligned to a larger accumulator: < 2^-4 of such a unit each, eight per group
    14      products aligned to the group's largest: < 2^-23 |largest| per dropped tail, seven per group, and the groups'
            largest products sum to <= sum |w||x|
    2       acc * ln 2 + bias in the epilogue (one if contracted to an fma)
    1       the reference's own fp32 read-back of its fp16 inputs (conv_ref.decode)

so F32_UNITS(K) = 3 K / 16 + 17: 29 for the box and class finals (K = 64), 20 for the keypoint finals (K = 16).  The fp32
finals, and only they, are bounded by that here instead of C_ACC; measured against it the worst is 4.7 / 29 = 0.16 (K = 64)
and 4.1 / 20 = 0.21 (K = 16).  Natural activations stay under C_ACC = 4 (0.876 at worst, tests/test_gpu_conv_candidates.py,
which is unchanged).  fp16 outputs pass with M_REL and C_ACC as they are: the fp16 rounding dominates (0.80 = 1 / (1 + M_REL)).

What the families cannot see: a load that IS selected away (it changes no bit, whatever it read) and one past the allocation
(no value to see); `range` bounds small outputs of large inputs only through C_ACC 2^-24 sum |w||x| (tests/test_act_craft.py).
"""
import ctypes as C
import time

import numpy as np
import pytest

import act_craft
import conv_ref
from irmv_detection_amd import capi
from irmv_detection_amd.engine import YoloEngine
from test_gpu_conv_candidates import C_ACC, M_REL, U32, bound, candidates, conv_ops, layer_table, ranges_for, read, run
from test_gpu_graph_ops import graph_ops, run_op

pytestmark = pytest.mark.gpu

assert (M_REL, C_ACC) == (0.25, 4.0)


def F32_UNITS(K):
    """fp32 roundings of a Detect final with K input channels, counted (module docstring, "Finding")."""
    return 3 * K // 16 + 17


FUSED_KINDS = ("c2f2", "c2f32", "bneck", "kpt3")
ENGINES = {   # tag -> (net, slots, tap blob)
    "224x1": (224, 1, False),      # the single-frame plan: c2f2, c2f32_*, bneck64_*, grouped / merged heads; maps 56 / 28 / 14 / 7
    "224x5": (224, 5, False),      # batched, shares 3 + 2: kpt3_*
    "64x3": (64, 3, False),        # every pixel a border pixel
    "tap224x1": (224, 1, True),
}
LOG = {}                           # tag -> lines for DESIGN.md's table, printed by the last test


# ---- engines and hooks ------------------------------------------------------------------------------------------------
class Rig:
    def __init__(self, tag, blob):
        net, slots, tap = ENGINES[tag]
        self.tag, self.blob = tag, act_craft.tap_blob(blob) if tap else blob
        self.e = YoloEngine(None, (1280, 1024), weights_blob=self.blob, net_size=net, num_slots=slots)
        self.N = slots
        self.share = -(-slots // self.e.num_streams)
        self.counts = [self.share, 1] if self.share > 1 else [1]
        self.ops = conv_ops(self.e)
        self.by_index = {o.op: o for o in self.ops}
        self.graph = graph_ops(self.e)
        self.table = layer_table(self.blob)
        self.shapes = {}

    def shape(self, name):
        if name not in self.shapes:
            s = (C.c_int * 3)()
            capi.check(self.e._L.irmv_engine_read_tap(self.e._h, 0, name.encode(), None, s))
            self.shapes[name] = tuple(s)
        return self.shapes[name]

    def dtype(self, name):
        return np.float32 if name.startswith("head.") else np.uint16

    def nan_tensor(self, name):
        """[N, H, W, C] of all-ones bytes: NaN in fp16 and in fp32."""
        dt = self.dtype(name)
        return np.full((self.N,) + self.shape(name), np.iinfo(np.uint16).max, np.uint16) if dt == np.uint16 else \
            np.full((self.N,) + self.shape(name), 0xFFFFFFFF, np.uint32).view(np.float32)

    def write(self, name, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.shape == (self.N,) + self.shape(name) and arr.dtype == self.dtype(name)
        capi.check(self.e._L.irmv_engine_write_tensor(self.e._h, name.encode(), 0, self.N, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def read(self, name):
        return read(self.e, name, 0, self.N)

    def close(self):
        self.e.__exit__(None, None, None)


@pytest.fixture(scope="module")
def rigs(blob):
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = Rig(tag, blob)
        return made[tag]
    yield get
    for r in made.values():
        r.close()


def op_io(rig, op):
    io = capi.OpIo()
    capi.check(rig.e._L.irmv_engine_op_io(rig.e._h, op, C.byref(io)))
    return io


def segs_of(op):
    """The declared inputs of a conv op record: [(key, segment)]."""
    return [(k, getattr(op, k)) for k in ("s0", "s1", "res") if getattr(op, k).C]


def touched(rig, op):
    """Every activation tensor a run of conv op `op` touches."""
    names = {s.tensor.decode() for _, s in segs_of(op)} | {op.out_tensor.decode()}
    if op.fused:
        names.add(op.fuse_tensor.decode())
    return sorted(names)


def stage(rig, names, declared, data, first, count):
    """Write every tensor of `names`: NaN everywhere, then data[name][slot] on the declared (name, coff, C) channel ranges of
    slots [first, first + count)."""
    for n in names:
        t = rig.nan_tensor(n)
        for name, coff, Cc in declared:
            if name == n:
                t[first:first + count, ..., coff:coff + Cc] = data[n][first:first + count, ..., coff:coff + Cc]
        rig.write(n, t)


def is_poison(a):
    return (a.view(np.uint32) == 0xFFFFFFFF) if a.dtype == np.float32 else (a == 0xFFFF)


def untouched_problems(rig, got, written, first, count):
    """After a run: everything of the touched tensors that the run was not to write is still all-ones.  got: {name: [N, H, W, C]},
    written: [(name, coff, C)] (a conv writes cout_pad channels: its padding channels are its own)."""
    bad = []
    for n, a in got.items():
        keep = np.ones(a.shape, bool)
        for name, coff, Cc in written:
            if name == n:
                keep[first:first + count, ..., coff:coff + Cc] = False
        if not is_poison(a)[keep].all():
            bad.append(f"{n}: something outside the run's output and the declared inputs changed, or an input was overwritten")
    return bad


# ---- one conv op on crafted inputs ------------------------------------------------------------------------------------
class Case:
    """Conv op `op` of a rig on inputs data = {tensor: [N, H, W, C] raw}: staging, running, the reference, the checks."""

    def __init__(self, rig, op, data, declared=None):
        self.rig, self.op, self.data = rig, op, data
        self.names = touched(rig, op)
        self.inputs = [(s.tensor.decode(), s.coff, s.C) for _, s in segs_of(op)]
        self.declared = declared if declared is not None else self.inputs
        w = rig.by_index[op.op]
        self.out = (op.fuse_tensor.decode(), op.fuse_coff, op.fuse_cout) if op.fused else (op.out_tensor.decode(), op.out_coff, op.cout)
        self.out_pad = (op.fuse_tensor.decode(), op.fuse_coff, op.fuse_cout_pad) if op.fused else (op.out_tensor.decode(), op.out_coff, op.cout_pad)
        self.f32 = bool(op.fused or op.out_f32)
        assert w.fused == w.tune_fused
        self._ref, self.bd4, self.worst4 = {}, {}, 0.0     # (bd4, worst4: an fp32 final against the C_ACC bound, for the log)

    def ref(self, slot):
        """(y, bound) of the op's visible output on one slot: its own output, or the head slice of the 1x1 it carries."""
        if slot not in self._ref:
            op, rig = self.op, self.rig
            ts = {n: conv_ref.decode(self.data[n][slot], n) for n in {s.tensor.decode() for _, s in segs_of(op)}}
            w, b = rig.table[op.layer.decode()]
            fuse = rig.table[op.fuse_layer.decode()] if op.fused else None
            with np.errstate(all="ignore"):
                r = conv_ref.op_forward(op, ts, w, b, fuse)
                bd = bound(r[0], r[1], op.out_f32)
                if op.out_f32:      # the fp32 finals: their own count of roundings, not C_ACC (module docstring, "Finding")
                    assert op.ks == 1 and op.act == 0 and not op.fused
                    self.bd4[slot], bd = bd, F32_UNITS(op.cin) * U32 * r[1]
                if op.fused:
                    w2 = np.abs(fuse[0].astype(np.float64))
                    prop = conv_ref.conv(bd, w2, np.zeros(len(w2)), 1, 0)[0]          # sum |w2| * bound of the fp16 input (layer_ratio)
                    self._ref[slot] = (r[2], C_ACC * U32 * r[3] + prop, r[0])
                else:
                    self._ref[slot] = (r[0], bd, r[0])
        return self._ref[slot]

    def go(self, T, cand, first, count):
        """Stage, poison the output, run -> the touched tensors as read back, or None if run_conv declined."""
        stage(self.rig, self.names, self.declared, self.data, first, count)
        if run(self.rig.e, self.op.op, T, cand, first, count) == capi.DECLINED:
            return None
        return {n: self.rig.read(n) for n in self.names}

    def out_of(self, got, first, count):
        n, coff, Cc = self.out
        return got[n][first:first + count, ..., coff:coff + Cc]

    def untouched(self, got, first, count):
        """Nothing but the output was written, and the declared inputs (outside the output) are as staged."""
        bad = untouched_problems(self.rig, got, [self.out_pad] + self.declared, first, count)
        n0, c0, C0 = self.out_pad
        for n, coff, Cc in self.declared:
            if not (n == n0 and coff < c0 + C0 and c0 < coff + Cc):
                if not np.array_equal(got[n][first:first + count, ..., coff:coff + Cc], self.data[n][first:first + count, ..., coff:coff + Cc]):
                    bad.append(f"{n}: the run changed its input")
        return bad

    def problems(self, got, first, count, finite=True):
        """The checks of (a) on a run's read-back -> (worst err / bound, [problems])."""
        bad = self.untouched(got, first, count)
        worst = 0.0
        for s in range(first, first + count):
            y, bd, y1 = self.ref(s)
            o = conv_ref.decode(self.out_of(got, s, 1)[0], self.out[0])
            w, p = act_craft.compare(o, y, bd, self.f32)
            if s in self.bd4 and np.isfinite(o).all():
                self.worst4 = max(self.worst4, float((np.abs(o - y) / self.bd4[s]).max()))
            worst = max(worst, w)
            bad += [f"slot {s}: {m}" for m in p]
            if finite and not np.isfinite(o).all():
                bad.append(f"slot {s}: {int((~np.isfinite(o)).sum())} outputs are not finite")
        return worst, bad


def conv_data(rig, op, rule, seed, top=None):
    """`range` inputs for conv op `op`: {tensor: [N, H, W, C]}, whole tensors (the declared ranges are cut out when staged)."""
    w, _ = rig.table[op.layer.decode()]
    t = act_craft.top_exponent(op.layer, w, bool(op.res.C)) if top is None else top
    names = sorted({s.tensor.decode() for _, s in segs_of(op)})
    return {n: act_craft.range_bits(seed * 131 + i, (rig.N,) + rig.shape(n), rule, t) for i, n in enumerate(names)}


def family(op):
    """The kernel family of a conv op, for the log: its chosen kernel's name up to the tile."""
    return op.kname.decode().split("_mt")[0].split("_nt")[0] + (" fp32 final" if op.out_f32 else "") + (" + carried 1x1" if op.fused else "")


def check_conv_range(rig, op, rule, seed, stats):
    """(a) for one conv op: its own choice on every range, every candidate bitwise the own choice.  -> [problems]"""
    case = Case(rig, op, conv_data(rig, op, rule, seed))
    for s in range(rig.N):     # the family's condition, on the inputs actually written
        y1 = case.ref(s)[2]
        assert np.isfinite(y1).all() and np.abs(y1).max() <= act_craft.REAL_LIMIT, (op.layer, rule, float(np.abs(y1).max()))
    bad = []
    for T in rig.counts:
        own = {}
        for first, count in ranges_for(T, rig.share, rig.N):
            got = case.go(T, -1, first, count)
            assert got is not None
            worst, p = case.problems(got, first, count)
            stats["worst"][op.layer.decode()] = max(stats["worst"].get(op.layer.decode(), 0.0), worst)
            if op.out_f32:
                stats["c4"][op.cin] = max(stats["c4"].get(op.cin, 0.0), case.worst4)
            bad += [(op.layer.decode(), rule, T, first, count, m) for m in p]
            own[(first, count)] = case.out_of(got, first, count).copy()
        first, count = (0, rig.share) if T == rig.share and T > 1 else (rig.N - 1, 1)
        cands = candidates(rig.e, op.op, T)
        stats["listed"] += len(cands)
        for i, cd in enumerate(cands):
            got = case.go(T, i, first, count)
            if got is None:
                stats["declined"] += 1
                continue
            stats["checked"] += 1
            if not np.array_equal(case.out_of(got, first, count), own[(first, count)]):
                bad.append((op.layer.decode(), rule, T, cd.name.decode(), "differs from the own choice"))
            bad += [(op.layer.decode(), rule, T, cd.name.decode(), m) for m in case.untouched(got, first, count)]
    return bad


def _log_conv(rig, what, stats, t0):
    fam = {}
    for op in rig.ops:
        r = stats["worst"].get(op.layer.decode())
        if r is not None:
            k = family(op)
            fam[k] = max(fam.get(k, (0.0, "")), (r, op.layer.decode()))
    lines = [f"[act craft {rig.tag} {what}] {len(stats['worst'])} conv ops; {stats['checked']} candidates checked + {stats['declined']} declined"
             f" = {stats['listed']} listed; {time.time() - t0:.1f} s"]
    lines += [f"    {k:28s} worst err/bound {r:.3f}  ({n})" for k, (r, n) in sorted(fam.items())]
    lines += [f"    fp32 finals, K = {K}: worst err / (C_ACC 2^-24 acc) {r:.3f}, bounded by F32_UNITS = {F32_UNITS(K)}: {r * C_ACC / F32_UNITS(K):.3f}"
              for K, r in sorted(stats["c4"].items())]
    lines += [f"      {n:26s} {r:.3f}" for n, r in stats["worst"].items()]
    LOG[(rig.tag, what)] = lines
    return lines


def new_stats():
    return {"worst": {}, "checked": 0, "declined": 0, "listed": 0, "c4": {}}


# ---- (a) range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["postsilu", "signed"])
@pytest.mark.parametrize("tag", ["224x1", "224x5", "64x3"])
def test_range_every_conv_op_and_candidate(rigs, capsys, tag, rule):
    rig, t0, stats, bad = rigs(tag), time.time(), new_stats(), []
    assert len(rig.ops) >= 40
    for i, op in enumerate(rig.ops):
        bad += check_conv_range(rig, op, rule, 7 + i, stats)
    with capsys.disabled():
        print("\n" + "\n".join(_log_conv(rig, f"range/{rule}", stats, t0)))
    assert not bad, bad[:10]
    assert stats["checked"] + stats["declined"] == stats["listed"] and stats["checked"] > 0
    assert len(stats["worst"]) == len({o.layer for o in rig.ops})


# ---- (b) ladder ---------------------------------------------------------------------------------------------------------
def test_ladder_every_activated_conv_op_and_candidate_on_the_tap_blob(rigs, capsys):
    rig, t0, stats, bad = rigs("tap224x1"), time.time(), new_stats(), []
    n_inf = 0
    for op in rig.ops:
        if op.act != 1:
            continue
        names = sorted({s.tensor.decode() for _, s in segs_of(op)})
        parts = max(act_craft.ladder_parts(rig.shape(n)) for n in names)
        cands = candidates(rig.e, op.op, 1)
        stats["listed"] += len(cands)
        ran = [None] * len(cands)
        for part in range(parts):
            data = {n: act_craft.tile_ladder((rig.N,) + rig.shape(n), part + 3 * i) for i, n in enumerate(names)}
            case = Case(rig, op, data)
            own = None
            for cand in [-1] + list(range(len(cands))):
                got = case.go(1, cand, 0, 1)
                if got is None:
                    assert cand >= 0 and ran[cand] in (None, False)
                    ran[cand] = False
                    continue
                if cand >= 0:
                    assert ran[cand] in (None, True)
                    ran[cand] = True
                worst, p = case.problems(got, 0, 1, finite=False)
                who = "own" if cand < 0 else cands[cand].name.decode()
                bad += [(op.layer.decode(), part, who, m) for m in p]
                stats["worst"][op.layer.decode()] = max(stats["worst"].get(op.layer.decode(), 0.0), worst)
                o = case.out_of(got, 0, 1)
                if own is None:
                    own = o.copy()
                    y = case.ref(0)[0]
                    n_inf += int(np.isposinf(y).sum())
                    if np.isposinf(y).any():        # +Inf in gives +Inf out (compare() has checked that these ARE +Inf)
                        assert np.isposinf(conv_ref.decode(o[0], case.out[0])[np.isposinf(y)]).all()
                elif not same_bits_and_nans([o], [own]):     # (a NaN's sign and payload are the kernel's own: 0 * Inf, Inf - Inf)
                    fo, fw = (o.view(np.float16), own.view(np.float16)) if o.dtype == np.uint16 else (o, own)
                    d = ~(np.isnan(fo) & np.isnan(fw)) & (o != own)
                    bad.append((op.layer.decode(), part, who, f"differs from the own choice in {int(d.sum())} elements that are not NaN in both, "
                                f"e.g. {fo[d][:3].tolist()} against {fw[d][:3].tolist()}"))
        stats["checked"] += ran.count(True)
        stats["declined"] += ran.count(False)
    with capsys.disabled():
        print("\n" + "\n".join(_log_conv(rig, "ladder", stats, t0)) + f"\n    +Inf outputs expected and found: {n_inf}")
    assert not bad, bad[:10]
    assert stats["checked"] + stats["declined"] == stats["listed"] and stats["checked"] > 0 and n_inf > 0


# ---- (c) NaN reach ------------------------------------------------------------------------------------------------------
def with_sites(rig, op, data, first, count):
    d = {n: v.copy() for n, v in data.items()}
    for s in range(first, first + count):
        act_craft.put_sites({n: v[s] for n, v in d.items()}, op, act_craft.nan_sites(op, seed=s))
    return d


@pytest.mark.parametrize("tag", ["224x1", "224x5", "64x3"])
def test_nan_reach_every_conv_op_and_candidate(rigs, capsys, tag):
    rig, t0, stats, bad = rigs(tag), time.time(), new_stats(), []
    reached = 0
    for i, op in enumerate(rig.ops):
        data = conv_data(rig, op, "postsilu", 900 + i)
        clean = Case(rig, op, data)
        for T in rig.counts:
            first, count = (0, rig.share) if T == rig.share and T > 1 else (rig.N - 1, 1)
            base = clean.go(T, -1, first, count)
            base_out = clean.out_of(base, first, count)
            case = Case(rig, op, with_sites(rig, op, data, first, count))
            want = np.stack([np.isnan(case.ref(s)[0]) for s in range(first, first + count)])
            if not op.fused:     # (a carried 1x1 spreads the field over its own output channels: the reference alone says where)
                field = np.stack([act_craft.nan_field(op, act_craft.nan_sites(op, seed=s)) for s in range(first, first + count)])
                assert np.array_equal(want, field), op.layer
            assert want.any()
            reached += int(want.sum())
            cands = candidates(rig.e, op.op, T)
            stats["listed"] += len(cands)
            for cand in [-1] + list(range(len(cands))):
                got = case.go(T, cand, first, count)
                who = "own" if cand < 0 else cands[cand].name.decode()
                if got is None:
                    stats["declined"] += 1
                    continue
                stats["checked"] += cand >= 0
                o = case.out_of(got, first, count)
                isn = np.isnan(o.view(np.float16)) if o.dtype == np.uint16 else np.isnan(o)
                if not np.array_equal(isn, want):
                    bad.append((op.layer.decode(), T, who, f"NaN set: {int(isn.sum())} outputs, {int(want.sum())} in the reference, "
                                f"{int((isn & ~want).sum())} outside it"))
                elif not np.array_equal(o[~want], base_out[~want]):
                    bad.append((op.layer.decode(), T, who, "an element the impulses do not reach differs from the impulse-free run"))
                bad += [(op.layer.decode(), T, who, m) for m in case.untouched(got, first, count)]
    LOG[(rig.tag, "nan")] = [f"[act craft {rig.tag} NaN reach] {len(rig.ops)} conv ops; {stats['checked']} candidates checked + {stats['declined']} declined = "
                            f"{stats['listed']} listed; {reached} NaN outputs expected; {time.time() - t0:.1f} s"]
    with capsys.disabled():
        print("\n" + LOG[(rig.tag, "nan")][0])
    assert not bad, bad[:10]
    assert stats["checked"] + stats["declined"] == stats["listed"] and stats["checked"] > 0


# ---- (d) fused ops --------------------------------------------------------------------------------------------------------
def fused_ops(rig):
    return [g for g in rig.graph if g.kind.decode() in FUSED_KINDS]


def fused_ranges(rig, kind):
    """(0, share), the remainder share, the last slot; a bneck launch is of the single-frame plan only."""
    r = [(rig.N - 1, 1)]
    if kind != "bneck" and rig.share > 1:
        r = [(0, rig.share)] + [(f, min(rig.share, rig.N - f)) for f in range(rig.share, rig.N, rig.share)] + r
    return list(dict.fromkeys(r))


class FusedCase:
    def __init__(self, rig, g, rule, seed, impulses):
        self.rig, self.g = rig, g
        io = op_io(rig, g.op)
        self.subs = [rig.by_index[io.sub[i]] for i in range(io.n_sub)]
        self.reads = [io.reads[i] for i in range(io.n_reads)]
        self.writes = [(io.writes[i].tensor.decode(), io.writes[i].coff, io.writes[i].C) for i in range(io.n_writes)]
        assert self.subs and self.reads and self.writes
        self.declared = [(s.tensor.decode(), s.coff, s.C) for s in self.reads]
        names = {n for n, _, _ in self.declared} | {n for n, _, _ in self.writes}
        for o in self.subs:
            names |= set(touched(rig, o))
        self.names = sorted(names)
        top = min(act_craft.top_exponent(o.layer, rig.table[o.layer.decode()][0], bool(o.res.C)) for o in self.subs)
        self.data = {n: act_craft.range_bits(seed * 17 + i, (rig.N,) + rig.shape(n), rule, top) for i, n in enumerate(sorted({n for n, _, _ in self.declared}))}
        if impulses:
            rng = np.random.Generator(np.random.PCG64(seed))
            for n, coff, Cc in self.declared:
                _, H, W, _ = self.data[n].shape
                for s in range(rig.N):
                    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (int(rng.integers(0, H)), int(rng.integers(0, W)))]:
                        self.data[n][s, y, x, coff + (0 if (y + x) % 2 else Cc - 1)] = act_craft.NAN_BITS

    def written(self, first, count):
        return [self.rig.read(n)[first:first + count, ..., coff:coff + Cc] for n, coff, Cc in self.writes]

    def layers(self, first, count, order=None):
        """The conv ops in order (a 1x1 its predecessor carries in its epilogue runs with it) -> the fused op's written ranges."""
        rig = self.rig
        stage(rig, self.names, self.declared, self.data, first, count)
        subs = self.subs if order is None else [self.subs[i] for i in order]
        prev = None
        for o in subs:
            if not (prev is not None and prev.fused and prev.fuse_layer == o.layer):
                assert run(rig.e, o.op, 1 if count == 1 else rig.share, -1, first, count) == capi.OK
            prev = o
        return self.written(first, count)

    def fused(self, first, count):
        rig = self.rig
        stage(rig, self.names, self.declared, self.data, first, count)
        run_op(rig.e, self.g.op, first, count)
        got = {n: rig.read(n) for n in self.names}
        keep = untouched_problems(rig, got, self.writes + [d for d in self.declared], first, count)
        # (the declared inputs: unchanged on the run's slots)
        for n, coff, Cc in self.declared:
            if not any(n == wn and coff < wc + wC and wc < coff + Cc for wn, wc, wC in self.writes):
                if not np.array_equal(got[n][first:first + count, ..., coff:coff + Cc], self.data[n][first:first + count, ..., coff:coff + Cc]):
                    keep.append(f"{n}: the run changed its input")
        return [got[n][first:first + count, ..., coff:coff + Cc] for n, coff, Cc in self.writes], keep


def same_bits_and_nans(a, b):
    """Bitwise outside the NaNs, and the same NaN set (two kernels may give a NaN different payloads)."""
    for x, y in zip(a, b):
        nx = np.isnan(x.view(np.float16)) if x.dtype == np.uint16 else np.isnan(x)
        ny = np.isnan(y.view(np.float16)) if y.dtype == np.uint16 else np.isnan(y)
        if not np.array_equal(nx, ny) or not np.array_equal(x[~nx], y[~ny]):
            return False
    return True


@pytest.mark.parametrize("tag", ["224x1", "224x5", "64x3"])
def test_fused_ops_are_their_layers_on_written_inputs(rigs, capsys, tag):
    rig, t0, bad, runs = rigs(tag), time.time(), [], {}
    for j, g in enumerate(fused_ops(rig)):
        kind = g.kind.decode()
        for k, (rule, impulses) in enumerate((("postsilu", False), ("signed", False), ("postsilu", True))):
            case = FusedCase(rig, g, rule, 300 + 10 * j + k, impulses)
            for first, count in fused_ranges(rig, kind):
                want = case.layers(first, count)
                got, keep = case.fused(first, count)
                assert not all(is_poison(w).all() for w in want), (g.layer, "the layers wrote nothing")
                if impulses:
                    assert any(is_poison(w).any() or np.isnan(w.view(np.float16) if w.dtype == np.uint16 else w).any() for w in want)
                if not same_bits_and_nans(got, want):
                    bad.append((g.layer.decode(), g.kname.decode(), rule, impulses, first, count, "differs from its layers"))
                bad += [(g.layer.decode(), g.kname.decode(), rule, impulses, first, count, m) for m in keep]
                runs[(kind, g.kname.decode())] = runs.get((kind, g.kname.decode()), 0) + 1
    LOG[(rig.tag, "fused")] = [f"[act craft {rig.tag} fused] " + ", ".join(f"{k[1]} x{v}" for k, v in sorted(runs.items())) + f"; {time.time() - t0:.1f} s"]
    with capsys.disabled():
        print("\n" + LOG[(rig.tag, "fused")][0])
    assert not bad, bad[:10]
    assert runs


def test_all_four_fused_kinds_are_met(rigs):
    """From irmv_engine_ops: the three engines together hold c2f2, c2f32 (all three modes), bneck (both) and kpt3 ops."""
    met, knames = set(), set()
    for tag in ("224x1", "224x5", "64x3"):
        for g in fused_ops(rigs(tag)):
            met.add(g.kind.decode())
            knames.add(g.kname.decode())
    assert met == set(FUSED_KINDS), met
    assert {"c2f2_fused", "c2f32_ab", "c2f32_a", "c2f32_b", "bneck64_a", "bneck64_b"} <= knames and any(k.startswith("kpt3_") for k in knames), knames


# ---- the hooks themselves -------------------------------------------------------------------------------------------------
def test_write_tensor_is_what_read_tensor_returns_and_no_read_back_recomputes_it(rigs):
    """After a step of an engine with a sparse head and gated box branches: what write_tensor wrote into a head tensor, a gated
    first conv's tensor and a tensor a fused kernel keeps on chip is what read_tensor returns, bit for bit, also after
    read_head; a size that is not the slot range's is refused."""
    rig = rigs("224x5")
    e = rig.e
    from irmv_detection_amd import frames
    for s in range(rig.N):
        e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
    e.submit(0, rig.N)
    e.wait()
    lazy = sorted({o.out_tensor.decode() for o in rig.ops if o.out_lazy})
    names = sorted({o.fuse_tensor.decode() for o in rig.ops if o.fused})[:1] + lazy[:2] + [rig.ops[0].out_tensor.decode()]
    wrote = {}
    for i, n in enumerate(names):
        if rig.dtype(n) == np.uint16:
            wrote[n] = act_craft.range_bits(40 + i, (rig.N,) + rig.shape(n), "signed")
        else:
            wrote[n] = np.random.Generator(np.random.PCG64(40 + i)).standard_normal((rig.N,) + rig.shape(n)).astype(np.float32)
        rig.write(n, wrote[n])
    e.read_head(0)
    e.read_head(rig.N - 1)
    for n, v in wrote.items():
        assert np.array_equal(rig.read(n), v), n
        part = read(e, n, 1, 2)
        assert np.array_equal(part, v[1:3]), n
    a = wrote[names[-1]]
    rc = e._L.irmv_engine_write_tensor(e._h, names[-1].encode(), 0, rig.N, a.ctypes.data_as(C.c_void_p), a.nbytes - 2)
    assert rc == capi.ERR_ARG
    rc = e._L.irmv_engine_write_tensor(e._h, names[-1].encode(), 1, 1, a.ctypes.data_as(C.c_void_p), a.nbytes)
    assert rc == capi.ERR_ARG
    assert e._L.irmv_engine_write_tensor(e._h, b"no.such.tensor", 0, 1, a.ctypes.data_as(C.c_void_p), a.nbytes) == capi.ERR_ARG
    capi.check(e._L.irmv_engine_write_tensor(e._h, names[-1].encode(), 2, 1, a[4:].ctypes.data_as(C.c_void_p), a[4:].nbytes))
    assert np.array_equal(rig.read(names[-1])[2], a[4]) and np.array_equal(rig.read(names[-1])[3], a[3])
    io = capi.OpIo()
    assert e._L.irmv_engine_op_io(e._h, rig.ops[0].op, C.byref(io)) == capi.ERR_ARG        # a conv op is no fused op


# ---- controls -------------------------------------------------------------------------------------------------------------
def _control_op(rig):
    """A 3x3 conv with 64 input channels and no carried 1x1."""
    return next(o for o in rig.ops if o.ks == 3 and o.s0.C == 64 and not o.s1.C and not o.fused and o.act == 1)


def test_control_a_nan_in_a_declared_input_fails_the_finiteness_check(rigs):
    rig = rigs("224x1")
    op = _control_op(rig)
    data = conv_data(rig, op, "postsilu", 1)
    case = Case(rig, op, data)
    assert not case.problems(case.go(1, -1, 0, 1), 0, 1)[1]
    n = op.s0.tensor.decode()
    data[n][0, op.Hin // 2, op.Win // 2, op.s0.coff + 5] = act_craft.NAN_BITS
    case = Case(rig, op, data)
    case._ref = {0: Case(rig, op, conv_data(rig, op, "postsilu", 1)).ref(0)}         # (the reference of the clean input: (a) expects finite outputs)
    _, p = case.problems(case.go(1, -1, 0, 1), 0, 1)
    assert any("not finite" in m for m in p), p


def test_control_an_undeclared_read_fails(rigs):
    """The test's copy of the op record narrowed by 16 channels of s0, those channels left poisoned: the kernel still reads
    them, and (a) fails."""
    rig = rigs("224x1")
    op = _control_op(rig)
    data = conv_data(rig, op, "postsilu", 2)
    narrowed = [(op.s0.tensor.decode(), op.s0.coff, op.s0.C - 16)] + [(s.tensor.decode(), s.coff, s.C) for k, s in segs_of(op) if k != "s0"]
    case = Case(rig, op, data, declared=narrowed)
    _, p = case.problems(case.go(1, -1, 0, 1), 0, 1)
    assert any("not finite" in m for m in p) and any("NaN set" in m for m in p), p


def test_control_swapped_sub_ops_fail(rigs):
    rig = rigs("224x1")
    g = next(g for g in fused_ops(rig) if g.kind == b"c2f32")
    case = FusedCase(rig, g, "postsilu", 5, False)
    got, keep = case.fused(0, 1)
    assert not keep and same_bits_and_nans(got, case.layers(0, 1))
    order = list(range(len(case.subs)))
    order[0], order[1] = order[1], order[0]
    assert not same_bits_and_nans(got, case.layers(0, 1, order))


def test_zz_log(capsys):
    """The tables of DESIGN.md "Crafted activations", as this run measured them."""
    with capsys.disabled():
        for key in sorted(LOG):
            print("\n".join(LOG[key][:1 + 12]))
