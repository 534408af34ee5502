"""Crafted activations for the per-layer checks (tests/test_gpu_act_craft.py): inputs somebody chose, written into the
engine's tensors, instead of what a forward pass of the synthetic blob on synthetic frames happens to leave there (every
activation in [-0.279, 18.5], median |a| 0.07 - 0.28, hardly an fp16 subnormal, pre-activations ~ N(0, 1.7^2)).

Everything here is raw storage: uint16 arrays of fp16 bits AT THE ACTIVATION SCALE (stored = log2(e) * real,
irmv_common.hpp), seeded, on the CPU.

    range     s * m * 2^k, k uniform over [-24, top], m uniform in [1, 2): subnormals up to ~4000 (top = 11).  Two sign rules:
              "postsilu" has negatives only in [-0.279 log2 e, 0), as the output of a SiLU has them; "signed" has both signs
              at every magnitude.  top_exponent() lowers top where a layer's outputs would leave fp16.
    ladder    a table of <= 4096 fp16 values: both signs, every exponent with 64 mantissas, and the special values.
    tap_blob  the same architecture with one-hot centre-tap weights: a layer's pre-activation IS an input value.
    nan_sites a handful of (y, x, channel) impulses per input segment and residual of a conv op.

The expectation of a run comes from conv_ref.op_forward on the same arrays: numpy propagates NaN (and 0 * Inf) through zero
weights as IEEE arithmetic and the MFMA do.  nan_field() states the same NaN set by index arithmetic alone.
"""
from __future__ import annotations

import numpy as np

from irmv_detection_amd import weights

LOG2E = 1.4426950408889634
NEG_LIMIT = 0.279 * LOG2E            # a SiLU output is >= -0.2785 (real units); stored: * log2 e
K_LO, K_HI = -24, 11                 # exponents of `range`: 2^-24 is the smallest fp16 subnormal, 2^11 * [1, 2) reaches 4096
REAL_LIMIT = 4.0e4                   # outputs beyond this (real units) come near fp16's 65504 at the stored scale (* log2 e)
NAN_BITS = 0xFFFF                    # what IRMV_RUN_POISON writes: a NaN in fp16, and in fp32 as 0xFFFFFFFF


def f16(bits: np.ndarray) -> np.ndarray:
    return np.asarray(bits, np.uint16).view(np.float16)


# ---- range ------------------------------------------------------------------------------------------------------------
def range_bits(seed, shape, rule: str, top: int = K_HI) -> np.ndarray:
    """uint16 [shape]: stored fp16 values s * m * 2^k.  rule "postsilu" or "signed"."""
    assert rule in ("postsilu", "signed") and K_LO <= top <= K_HI
    rng = np.random.Generator(np.random.PCG64(seed))
    k = rng.integers(K_LO, top + 1, size=shape)
    m = 1.0 + rng.random(size=shape)
    neg = rng.random(size=shape) < 0.5
    v = np.ldexp(m, k).astype(np.float16)            # (rounds to the subnormal grid below 2^-14)
    if rule == "postsilu":
        neg &= v.astype(np.float64) <= NEG_LIMIT
    v = np.where(neg, -v, v).astype(np.float16)
    assert np.isfinite(v).all()
    return v.view(np.uint16)


def top_exponent(spec, w: np.ndarray, residual: bool) -> int:
    """The top exponent of `range` for a conv layer with weights w (OHWI): the largest k <= 11 at which six standard
    deviations of its pre-activation (+ the residual's largest value) stay under REAL_LIMIT.  With x = m 2^k, k uniform
    over n = top + 25 exponents and m uniform in [1, 2), E x^2 = (7 / 3) (4^(top + 1) - 4^-24) / (3 n) at the stored scale;
    the pre-activation of output o has variance sum_i w_oi^2 E x^2 (independent inputs, the mean term is smaller).  Six
    sigma over < 10^6 outputs; tests/test_act_craft.py checks the condition itself on the float64 reference."""
    w2 = float((np.asarray(w, np.float64) ** 2).reshape(w.shape[0], -1).sum(axis=1).max())
    for top in range(K_HI, K_LO, -1):
        n = top - K_LO + 1
        ex2 = (7.0 / 3.0) * (4.0 ** (top + 1)) / (3.0 * n) / LOG2E ** 2          # real units
        ex1 = 1.5 * (2.0 ** (top + 1)) / n / LOG2E                               # E |x|: "postsilu" inputs have a mean, and sum_i w_oi
        peak = 6.0 * np.sqrt(w2 * ex2) + 3.0 * np.sqrt(w2) * ex1 + (2.0 ** (top + 1) / LOG2E if residual else 0.0)   # is ~ N(0, 1) sqrt(w2)
        if peak <= REAL_LIMIT:
            return top
    raise AssertionError(spec)


# ---- ladder -----------------------------------------------------------------------------------------------------------
def ladder() -> np.ndarray:
    """uint16 [n <= 4096]: both signs x every exponent field 0..30 x 64 evenly spaced mantissas, then the special values:
    +-0, the smallest and largest subnormal, +-65504 / log2 e rounded inward (the largest real 65504 ... at the stored
    scale), +-65504 and +Inf.  -Inf and NaN are no SiLU output and no residual sum: y * rcp(1 + exp2(+inf)) is -Inf * 0."""
    e, m = np.meshgrid(np.arange(31, dtype=np.uint16), np.arange(64, dtype=np.uint16) * 16, indexing="ij")
    pos = ((e << 10) | m).reshape(-1).astype(np.uint16)
    body = np.concatenate([pos, pos | 0x8000])
    big = np.float16(65504.0 / LOG2E)
    if float(big) > 65504.0 / LOG2E:
        big = np.nextafter(big, np.float16(0))
    b = int(big.view(np.uint16))
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, b, b | 0x8000, 0x7BFF, 0xFBFF, 0x7C00], np.uint16)
    t = np.array(list(dict.fromkeys(np.concatenate([body, special]).tolist())), np.uint16)
    assert len(t) <= 4096
    return t


def tile_ladder(shape, part: int = 0) -> np.ndarray:
    """The ladder laid over a tensor [..., C] in memory order, each repetition rotated by 7 entries more than the last, so
    that an entry meets different channels and columns (the table's length and the channel counts share factors).  A tensor
    smaller than the table takes it in ladder_parts(shape) parts: part p starts at entry p * size."""
    t = ladder()
    n = int(np.prod(shape))
    i = np.arange(n) + part * n
    return t[(i + (i // len(t)) * 7) % len(t)].reshape(shape)


def ladder_parts(shape) -> int:
    return -(-len(ladder()) // int(np.prod(shape)))


# ---- comparing a run with its reference -------------------------------------------------------------------------------
def compare(out, y_ref, bd, f32: bool):
    """out (real units, decoded as read_tap does) against the float64 reference under the per-element bound bd ->
    (worst err / bound over the finite reference values, problems: list of str).  A reference NaN must be a NaN and nothing
    else may be one; a reference Inf must be that Inf; an fp16 output whose reference lies beyond the format (>= 65520 at
    the stored scale: rounds to Inf) must be that Inf, and one between 65504 and 65520 may be either."""
    out, y = np.asarray(out, np.float64), np.asarray(y_ref, np.float64)
    problems = []
    if not np.array_equal(np.isnan(out), np.isnan(y)):
        problems.append(f"NaN set differs: {int(np.isnan(out).sum())} NaN outputs, {int(np.isnan(y).sum())} in the reference")
    stored = np.abs(y) * LOG2E
    half = np.bool_(not f32)
    over = np.isinf(y) | (half & (stored >= 65520.0) & ~np.isnan(y))
    edge = ~over & ~np.isnan(y) & half & (stored > 65504.0)
    if not np.array_equal(out[over], np.sign(y[over]) * np.inf):
        problems.append("an output whose reference is infinite, or beyond fp16, is not that infinity")
    fin = ~over & ~edge & ~np.isnan(y) & ~np.isnan(out)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(out[fin] - y[fin]) / np.asarray(bd, np.float64)[fin]
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        problems.append(f"err / bound {worst:.3f}")
    return worst, problems


# ---- tap blob ---------------------------------------------------------------------------------------------------------
def tap_blob(blob: bytes) -> bytes:
    """The same architecture; every activated conv layer: w[o, centre, centre, o % cin] = 1, zero elsewhere; every bias 0.
    The pre-activation of output channel o is input channel o % cin of the centre-tap pixel, exactly."""
    hdr, layers = weights.parse_blob(blob)
    specs, tensors = [], []
    for sp, w, b in layers:
        w = w.copy()
        if sp.act == 1 and sp.groups == 1:
            w[:] = 0
            o = np.arange(sp.cout)
            w[o, sp.k // 2, sp.k // 2, o % sp.cin] = 1
        specs.append(sp)
        tensors.append((w, np.zeros_like(b)))
    return weights.build_blob(specs, tensors, hdr["nc"], hdr["nk"], hdr["backbone"])


# ---- NaN reach --------------------------------------------------------------------------------------------------------
def seg_hw(op, seg):
    """Rows x columns of the tensor behind an input segment of conv op `op` (half the conv's input where shift is 1)."""
    return op.Hin >> seg.shift, op.Win >> seg.shift


def nan_sites(op, seed: int = 0):
    """{"s0" | "s1" | "res": [(y, x, c)]}: impulses in the coordinates of each segment's own tensor (c: channel of the tensor).
    Pixels: the four corners, the centre, two seeded interior pixels.  Channels: the first and last of s0, the first of s1,
    one of res -- dealt over the pixels in turn."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))

    def pixels(H, W):
        p = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
        for _ in range(2):   # (always drawn, so that the sequence does not depend on the map's size)
            u, v = rng.random(), rng.random()
            p.append((1 + int(u * (H - 2)) if H > 2 else H // 2, 1 + int(v * (W - 2)) if W > 2 else W // 2))
        return list(dict.fromkeys(p))

    out = {}
    chans = {"s0": [op.s0.coff, op.s0.coff + op.s0.C - 1]}
    if op.s1.C:
        chans["s1"] = [op.s1.coff]
    if op.res.C:
        chans["res"] = [op.res.coff + int(rng.integers(0, op.cout))]
    for key, cs in chans.items():
        seg = getattr(op, key)
        H, W = (op.Hout, op.Wout) if key == "res" else seg_hw(op, seg)
        out[key] = [(y, x, cs[i % len(cs)]) for i, (y, x) in enumerate(pixels(H, W))]
    return out


def nan_field(op, sites) -> np.ndarray:
    """bool [Hout, Wout, cout]: the outputs of conv op `op` that an impulse of `sites` reaches, by index arithmetic alone.  An
    input impulse at conv-input pixel (iy, ix) -- a shift segment's tensor pixel stands for the 2 x 2 block it is upsampled
    to -- reaches EVERY output channel (a NaN times any weight, zero included, is NaN) of the output pixels (oy, ox) with
    oy * stride - k // 2 + ky = iy for a tap ky in [0, k), likewise in x.  A residual impulse reaches its own element only."""
    k, s, p = op.ks, op.stride, op.ks // 2
    out = np.zeros((op.Hout, op.Wout, op.cout), bool)
    for key in ("s0", "s1"):
        seg = getattr(op, key)
        for y, x, _ in sites.get(key, []):
            f = 1 << seg.shift
            for iy in range(y * f, y * f + f):
                for ix in range(x * f, x * f + f):
                    oys = [(iy + p - ky) // s for ky in range(k) if (iy + p - ky) % s == 0 and 0 <= (iy + p - ky) // s < op.Hout]
                    oxs = [(ix + p - kx) // s for kx in range(k) if (ix + p - kx) % s == 0 and 0 <= (ix + p - kx) // s < op.Wout]
                    for oy in oys:
                        for ox in oxs:
                            out[oy, ox, :] = True
    for y, x, c in sites.get("res", []):
        out[y, x, c - op.res.coff] = True
    return out


def put_sites(tensors: dict, op, sites) -> None:
    """Write the impulses (NaN bits) into raw tensors {name: uint16 [H, W, C]} in place."""
    for key, lst in sites.items():
        t = tensors[getattr(op, key).tensor.decode()]
        for y, x, c in lst:
            t[y, x, c] = NAN_BITS
