"""tests/act_craft.py on the CPU: what the crafted inputs of tests/test_gpu_act_craft.py are, and that the per-layer bound is
tight enough on them to see a wrong SiLU.

The tightness control, in figures (tap blob: acc = |x|, real units).  bound() at a large output y ~ x is
(1.25 * 2^-11 + 4 * 2^-24) |y|: a SiLU off by a relative 2^-9 is 3.2 times that.  A SiLU that flushes an fp16-subnormal result
to zero is off by |silu(y)| = |y| e^-|y|, against C_ACC 2^-24 |y| + 2^-24 ln 2 + ...: it leaves the bound where
e^-|y| > 2.4e-7, i.e. for -15.2 < y < -12.7 (below -12.7 the result, at the stored scale, is subnormal).  At y = -17 itself
the result is 7.0e-7 and the accumulation term alone 4.1e-6: that element stays inside, whatever the kernel returns for it --
C_ACC 2^-24 sum |w||x| scales with the INPUT, and no bound of this form sees a SiLU output that is 2^-22 of its input.
"""
import numpy as np
import pytest

import act_craft
import conv_ref
from irmv_detection_amd import arch, capi, weights
from test_gpu_conv_candidates import bound


def fake_op(ks, stride, act, Hin, Win, cout, s0, s1=None, res=None):
    """A capi.ConvOp as irmv_engine_conv_ops would fill it; segments (tensor, coff, C, shift)."""
    op = capi.ConvOp()
    op.ks, op.stride, op.act, op.cout, op.cout_pad = ks, stride, act, cout, -(-cout // 16) * 16
    op.Hin, op.Win, op.Hout, op.Wout = Hin, Win, Hin // stride, Win // stride
    for key, s in (("s0", s0), ("s1", s1), ("res", res)):
        if s:
            seg = getattr(op, key)
            seg.tensor, seg.coff, seg.C, seg.shift = s[0].encode(), s[1], s[2], s[3]
    op.cin = op.s0.C + op.s1.C
    return op


REACH = [   # (id, op, tensor shapes)
    ("3x3-res", fake_op(3, 1, 1, 7, 9, 16, ("t", 0, 16, 0), None, ("cat", 16, 16, 0)), {"t": (7, 9, 16), "cat": (7, 9, 48)}),
    ("3x3-s2", fake_op(3, 2, 1, 8, 6, 16, ("a", 8, 16, 0)), {"a": (8, 6, 32)}),
    ("1x1-up-cat", fake_op(1, 1, 1, 6, 8, 32, ("p5", 0, 16, 1), ("p4", 8, 16, 0)), {"p5": (3, 4, 16), "p4": (6, 8, 24)}),
    ("3x3-up-cat", fake_op(3, 1, 0, 4, 4, 16, ("p5", 0, 8, 1), ("p4", 0, 8, 0)), {"p5": (2, 2, 8), "p4": (4, 4, 8)}),
    ("3x3-2x2", fake_op(3, 1, 1, 2, 2, 16, ("a", 0, 16, 0)), {"a": (2, 2, 16)}),
    ("3x3-s2-2x2", fake_op(3, 2, 1, 4, 4, 16, ("a", 0, 16, 0)), {"a": (4, 4, 16)}),
]


@pytest.mark.parametrize("tag,op,shapes", REACH, ids=[r[0] for r in REACH])
def test_reference_nan_set_is_the_receptive_field(tag, op, shapes):
    """conv_ref.op_forward on a finite `range` input with the impulses of nan_sites written in: its NaN set is nan_field(),
    the k x k window at stride through the 2x upsample of a shift segment, and the same element for the residual.  Half of the
    weights are zero: a NaN passes a zero weight."""
    rng = np.random.Generator(np.random.PCG64(5))
    raw = {n: act_craft.range_bits(11 + i, s, "postsilu", 4) for i, (n, s) in enumerate(shapes.items())}
    sites = act_craft.nan_sites(op, seed=3)
    assert set(sites) == {"s0"} | ({"s1"} if op.s1.C else set()) | ({"res"} if op.res.C else set())
    for key, lst in sites.items():
        seg = getattr(op, key)
        H, W = shapes[seg.tensor.decode()][:2]
        px = {(y, x) for y, x, _ in lst}
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)} <= px
        assert all(seg.coff <= c < seg.coff + seg.C for _, _, c in lst)
    assert {c for _, _, c in sites["s0"]} == {op.s0.coff, op.s0.coff + op.s0.C - 1}
    w = rng.standard_normal((op.cout, op.ks, op.ks, op.cin)).astype(np.float16)
    w[rng.random(w.shape) < 0.5] = 0
    b = rng.standard_normal(op.cout).astype(np.float32)
    clean = conv_ref.op_forward(op, {n: conv_ref.decode(v, n) for n, v in raw.items()}, w, b)[0]
    assert np.isfinite(clean).all()
    act_craft.put_sites(raw, op, sites)
    y = conv_ref.op_forward(op, {n: conv_ref.decode(v, n) for n, v in raw.items()}, w, b)[0]
    field = act_craft.nan_field(op, sites)
    assert field.any() and (op.Hout * op.Wout <= 16 or not field.all())     # (on the smallest maps the impulses reach everything)
    assert np.array_equal(np.isnan(y), field)
    assert np.array_equal(y[~field], clean[~field])


def test_ladder_coverage():
    t = act_craft.ladder()
    assert 3968 < len(t) <= 4096 and len(set(t.tolist())) == len(t)
    v = act_craft.f16(t)
    assert not np.isnan(v).any() and np.isinf(v).sum() == 1 and v[np.isinf(v)][0] > 0
    for sign in (0, 0x8000):
        for e in range(31):
            m = {int(b) & 0x3FF for b in t if (int(b) & 0x8000) == sign and ((int(b) >> 10) & 31) == e}
            assert len(m) >= 64, (sign, e)
    big = 65504.0 / act_craft.LOG2E
    for want in (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7C00):
        assert want in t
    pos = v[np.isfinite(v) & (v > 0)].astype(np.float64)
    inward = pos[pos <= big].max()
    assert inward > big - 32 and -inward in v.astype(np.float64)        # (fp16 step 32 there)
    assert act_craft.ladder_parts((7, 7, 256)) == 1 and act_craft.ladder_parts((7, 7, 16)) == 6
    tiled = act_craft.tile_ladder((56, 56, 48))
    inf_ch = {int(i) % 48 for i in np.flatnonzero(tiled.reshape(-1) == 0x7C00)}
    assert len(inf_ch) > 16 and max(inf_ch) >= 40                        # +Inf meets many channels, the last eight among them
    got = set()
    for p in range(6):
        got |= set(act_craft.tile_ladder((7, 7, 16), p).reshape(-1).tolist())
    assert got == set(t.tolist())


def test_range_families():
    for rule in ("postsilu", "signed"):
        v = act_craft.f16(act_craft.range_bits(1, (64, 64, 32), rule)).astype(np.float64)
        a = np.abs(v)
        assert np.isfinite(v).all() and a.max() > 4000 and a.max() < 8192
        sub = (a > 0) & (a < 2.0 ** -14)
        assert 0.2 < sub.mean() < 0.35                                   # exponents -24 .. -15 of 36
        assert (v < 0).any()
        if rule == "postsilu":
            assert v.min() >= -act_craft.NEG_LIMIT
        else:
            assert v.min() < -4000
    assert np.abs(act_craft.f16(act_craft.range_bits(1, (64, 64), "signed", 3)).astype(np.float64)).max() < 16


def _layer_cases(net):
    """(spec, Hin, Win, residual) of every conv layer of the C2f network but model.0.conv at this net size."""
    hw = arch.conv_out_hw(net)
    for sp in arch.conv_specs():
        if sp.name == "model.0.conv":
            continue
        idx = int(sp.name.split(".")[1])
        res = idx in (2, 4, 6, 8) and ".m." in sp.name and sp.name.endswith("cv2")     # the backbone's bottlenecks have the shortcut
        yield sp, hw[sp.name] * sp.stride, hw[sp.name] * sp.stride, res


@pytest.mark.parametrize("net", [224, 64])
def test_range_keeps_every_layer_of_the_synthetic_blob_in_fp16(net):
    """The condition of the `range` family on every conv op shape of the engines of tests/test_gpu_act_craft.py: with the
    synthetic blob and top_exponent(), the float64 reference alone has no output beyond +-4.0e4 (real units) and none that is
    not finite.  (The merged first-stage Detect convs of single-frame engines are these layers side by side.)"""
    table = {sp.name: (w, b) for sp, w, b in weights.parse_blob(weights.synthetic_blob(0))[1]}
    lowered = {}
    for i, (sp, H, W, res) in enumerate(_layer_cases(net)):
        w, b = table[sp.name]
        top = act_craft.top_exponent(sp, w, res)
        if top < act_craft.K_HI:
            lowered[sp.name] = top
        for j, rule in enumerate(("postsilu", "signed")):
            x = conv_ref.decode(act_craft.range_bits(100 + 2 * i + j, (H, W, sp.cin), rule, top), "x")
            r = conv_ref.decode(act_craft.range_bits(500 + 2 * i + j, (H // sp.stride, W // sp.stride, sp.cout), rule, top), "r") if res else None
            y, _ = conv_ref.conv(x, w, b, sp.stride, sp.act, r)
            assert np.isfinite(y).all() and np.abs(y).max() <= act_craft.REAL_LIMIT, (sp.name, rule, float(np.abs(y).max()))
    assert all(t >= 8 for t in lowered.values()), lowered        # (the family still reaches the hundreds everywhere)


def _tap_case():
    """One 1x1 layer of the tap blob on the ladder: (reference y, acc, the fp16 store of y as read back)."""
    blob = act_craft.tap_blob(weights.synthetic_blob(0))
    table = {sp.name: (sp, w, b) for sp, w, b in weights.parse_blob(blob)[1]}
    sp, w, b = table["model.9.cv1"]
    op = fake_op(1, 1, 1, 7, 7, sp.cout, ("8", 0, sp.cin, 0))
    x = conv_ref.decode(act_craft.tile_ladder((7, 7, sp.cin)), "8")
    with np.errstate(all="ignore"):
        y, acc = conv_ref.op_forward(op, {"8": x}, w, b)
        good = (y * act_craft.LOG2E).astype(np.float16).astype(np.float32) * conv_ref.LN2
    return x, y, acc, good


def test_tap_blob_makes_the_preactivation_an_input_value():
    blob = weights.synthetic_blob(0)
    tap = act_craft.tap_blob(blob)
    for (sp, w, b), (sp0, w0, _) in zip(weights.parse_blob(tap)[1], weights.parse_blob(blob)[1]):
        assert sp == sp0 and not b.any()
        if sp.act == 1 and sp.groups == 1:
            assert (w != 0).sum() == sp.cout and (w.reshape(sp.cout, -1).sum(axis=1) == 1).all()
            assert all(w[o, sp.k // 2, sp.k // 2, o % sp.cin] == 1 for o in range(sp.cout))
        else:
            assert np.array_equal(w, w0)
    x, y, acc, good = _tap_case()
    fin = np.isfinite(x).all(axis=-1)
    assert np.array_equal(acc[fin][:, :128], np.abs(x.astype(np.float64))[fin][:, :128])      # cout 128 of cin 256: o % cin = o
    with np.errstate(all="ignore"):
        assert np.array_equal(y[fin][:, :128], conv_ref.silu(x.astype(np.float64))[fin][:, :128])


def test_bound_is_tight_on_the_tap_blob():
    """The red control: an exact SiLU stored to fp16 is inside the existing bound() on the whole ladder; one that is off by a
    relative 2^-9 at |y| > 16 and one that returns 0 for a subnormal result both leave it (module docstring)."""
    x, y, acc, good = _tap_case()
    with np.errstate(all="ignore"):
        bd = bound(y, acc, False)
        worst, problems = act_craft.compare(good, y, bd, False)
        assert not problems and worst <= 1.0 / 1.25 + 1e-3, (worst, problems)
        xs = np.broadcast_to(x[..., :128].astype(np.float64), y.shape) if y.shape[-1] == 128 else None
        assert xs is not None
        off = np.where(np.abs(xs) > 16, good * (1.0 + 2.0 ** -9), good)
        w1, p1 = act_craft.compare(off, y, bd, False)
        assert w1 > 2.0 and p1
        stored = np.abs(y) * act_craft.LOG2E
        flushed = np.where(stored < 2.0 ** -14, 0.0, good)
        r = np.abs(flushed - y) / bd
        seen = np.isfinite(y) & (r > 1.0)
        assert seen.any()
        ys = xs[seen & (xs < -1.0)]                                     # (small inputs of either sign have subnormal results too, and are seen)
        assert ys.size and ys.max() < -12.5 and ys.min() > -15.5                    # where a flushed subnormal is seen ...
        at17 = np.isfinite(y) & (np.abs(xs + 17.0) < 0.1)
        assert at17.any() and (r[at17] < 0.25).all()                    # ... and y = -17 is not: 7.0e-7 against 4.1e-6
        _, p2 = act_craft.compare(flushed, y, bd, False)
        assert p2
