"""A seeded checkpoint that looks like a trained one before BatchNorm is folded, under Ultralytics names.

Test infrastructure.  weights.synthetic_tensors draws every weight i.i.d. Gaussian with one gain per layer.  A BN-folded
checkpoint is different: per-output-channel scales over orders of magnitude, dead channels, negative gains, biases far
larger than sum |w x|, folded weights in the fp16 subnormal range.  make() builds such a state-dict (YOLOv8n C2f backbone):

  * every activated layer of arch.conv_specs: <module>.conv.weight (OIHW, Gaussian / sqrt(fan_in), no conv bias) and
    <module>.bn.{weight, bias, running_mean, running_var}, eps = 1e-3; the nine Detect finals: <layer>.weight / .bias.
  * running statistics are MEASURED: a float64 forward (conv -> batch-norm(eval) -> SiLU), layer by layer over four
    frames.synthetic_frame at `net`, sets each layer's mean and variance to what its conv output has on those frames, so
    the post-BN pre-activation of channel c is about N(beta_c, gamma_c^2) whatever came before.
  * |gamma| = 2^u, u uniform in [-12, 1], random sign.  One channel in 32 (at least one per layer) has gamma = 0 exactly;
    across the layers these sit at the first channel, the last channel and both sides of a multiple of 16.
  * beta ~ N(0, 1); on the dead channels it cycles through -6, 0, +6.
  * the class bias is chosen so that every calibration frame has between 1 and 300 (anchor, class) candidates at
    score_thr = 0.25 under the float64 forward (tests/test_checkpoint.py asserts it).

fold() is the BatchNorm fusion in float64; expected_tensors() is what a blob imported from a file of a given stored dtype
must hold.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from irmv_detection_amd import arch, frames, weights
from onnx_files import stem
from torch_ref import TorchNet

EPS = 1e-3
N_CALIB = 4
SCORE_THR = 0.25
TARGET_CANDIDATES = 40          # per frame, of the 1 .. 300 the class bias has to land in


def module(sp: arch.ConvSpec) -> str:
    return sp.name[:-5] if sp.name.endswith(".conv") else sp.name


def is_final(sp: arch.ConvSpec) -> bool:
    return sp.act == arch.ACT_NONE


def calib_inputs(net: int) -> np.ndarray:
    """[N_CALIB, 3, net, net] float32: the frames the running statistics are measured on."""
    from oracle import oracle
    oracle.build()
    return np.stack([oracle.preprocess(frames.synthetic_frame(i), net) for i in range(N_CALIB)])


def dead_channels(layer_index: int, cout: int):
    """max(1, cout // 32) channels: the first, the last, and both sides of every multiple of 16, starting at another of
    them in every layer."""
    cand = [0, cout - 1] + [c for m in range(16, cout, 16) for c in (m - 1, m)]
    cand = list(dict.fromkeys(cand[layer_index % len(cand):] + cand[:layer_index % len(cand)]))
    return sorted(cand[:max(1, cout // 32)])


class UnfusedNet(TorchNet):
    """float64 forward of the checkpoint as it is: conv (no bias) -> batch-norm (eval) -> SiLU; the finals conv + bias.
    With measure=True, a batch [B, 3, N, N] goes through and each layer's running statistics are set, the first time the
    layer runs, to the mean and (biased) variance of its own conv output over the batch."""

    def __init__(self, ckpt: dict, measure: bool = False):
        self.ck, self.measure = ckpt, measure
        self.nc = ckpt["model.22.cv3.0.2.weight"].shape[0]
        self.nk = ckpt["model.22.cv4.0.2.weight"].shape[0] if "model.22.cv4.0.2.weight" in ckpt else 0
        self.backbone = arch.BACKBONE_C2F
        self.specs = {sp.name: sp for sp in arch.conv_specs(self.nc, self.nk)}
        self.taps = {}

    def _t(self, key):
        return torch.from_numpy(np.asarray(self.ck[key], np.float64))

    def conv(self, name, x):
        if x.dim() == 5:            # (TorchNet.forward adds the batch axis itself)
            x = x[0]
        sp = self.specs[name]
        if is_final(sp):
            return F.conv2d(x, self._t(name + ".weight"), self._t(name + ".bias"), stride=sp.stride, padding=sp.k // 2)
        m = module(sp)
        y = F.conv2d(x, self._t(m + ".conv.weight"), None, stride=sp.stride, padding=sp.k // 2)
        if self.measure and m + ".bn.running_mean" not in self.ck:
            self.ck[m + ".bn.running_mean"] = y.mean(dim=(0, 2, 3)).numpy().astype(np.float32)
            self.ck[m + ".bn.running_var"] = y.var(dim=(0, 2, 3), unbiased=False).numpy().astype(np.float32)
        y = F.batch_norm(y, self._t(m + ".bn.running_mean"), self._t(m + ".bn.running_var"), self._t(m + ".bn.weight"),
                         self._t(m + ".bn.bias"), training=False, eps=EPS)
        return F.silu(y)


class FusedNet(TorchNet):
    """TorchNet on a dict of fused convs {<stem>.weight OIHW, <stem>.bias} in a dtype of choice (no rounding to fp16)."""

    def __init__(self, fused: dict, dtype=torch.float64):
        self.nc = fused["model.22.cv3.0.2.weight"].shape[0]
        self.nk = fused["model.22.cv4.0.2.weight"].shape[0] if "model.22.cv4.0.2.weight" in fused else 0
        self.backbone = arch.BACKBONE_C2F
        self.p = {sp.name: (sp, torch.from_numpy(np.asarray(fused[stem(sp) + ".weight"])).to(dtype),
                            torch.from_numpy(np.asarray(fused[stem(sp) + ".bias"])).to(dtype))
                  for sp in arch.conv_specs(self.nc, self.nk)}
        self.taps = {}


def n_candidates(head: np.ndarray, nc: int) -> int:
    """(anchor, class) pairs whose score passes SCORE_THR (sigmoid(l) > t <=> l > log(t / (1 - t)))."""
    return int((np.asarray(head)[:, 64:64 + nc] > np.log(SCORE_THR / (1.0 - SCORE_THR))).sum())


def _make(seed: int, nc: int, nk: int, net: int) -> dict:
    rng = np.random.Generator(np.random.PCG64(seed))
    specs = arch.conv_specs(nc, nk)
    ck, n_dead = {}, 0
    for li, sp in enumerate(specs):
        fan_in = sp.cin * sp.k * sp.k
        w = (rng.standard_normal((sp.cout, sp.cin, sp.k, sp.k)) / np.sqrt(fan_in)).astype(np.float32)
        if not is_final(sp):
            m = module(sp)
            gamma = np.exp2(rng.uniform(-12.0, 1.0, sp.cout)) * rng.choice([-1.0, 1.0], sp.cout)
            beta = rng.standard_normal(sp.cout)
            for c in dead_channels(li, sp.cout):
                gamma[c], beta[c] = 0.0, (-6.0, 0.0, 6.0)[n_dead % 3]
                n_dead += 1
            ck[m + ".conv.weight"] = w
            ck[m + ".bn.weight"], ck[m + ".bn.bias"] = gamma.astype(np.float32), beta.astype(np.float32)
            continue
        b = rng.standard_normal(sp.cout)
        branch = sp.name.split(".")[2]
        if branch == "cv2":          # DFL logits: decaying bias, as weights.synthetic_tensors
            w, b = w * 1.68, b * 0.3 - 0.4 * (np.arange(sp.cout) % arch.REG_MAX)
        elif branch == "cv3":        # class logits; the common offset is chosen below
            w, b = w * 1.68, b * 0.2
        else:                        # keypoints: an armor-like quad around the anchor
            w, b = w * 0.25, 0.25 + np.array(weights.KPT_BASE).reshape(-1)[:sp.cout] / 2.0 + 0.02 * b
        ck[sp.name + ".weight"], ck[sp.name + ".bias"] = w.astype(np.float32), b.astype(np.float32)
    x = torch.from_numpy(calib_inputs(net).astype(np.float64))
    UnfusedNet(ck, measure=True).forward(x)                 # sets every running_mean / running_var
    # class bias: the offset at which the frames have TARGET_CANDIDATES candidates on average
    un = UnfusedNet(ck)
    t = np.log(SCORE_THR / (1.0 - SCORE_THR))
    kth = [np.sort(un.forward(x[i]).numpy()[:, 64:64 + nc].reshape(-1))[-TARGET_CANDIDATES] for i in range(N_CALIB)]
    shift = np.float32(t - float(np.mean(kth)) + 1e-3)
    for i in range(3):
        ck[f"model.22.cv3.{i}.2.bias"] = (ck[f"model.22.cv3.{i}.2.bias"] + shift).astype(np.float32)
    return ck


@functools.lru_cache(maxsize=4)
def _cached(seed, nc, nk, net):
    return _make(seed, nc, nk, net)


def make(seed: int, nc: int = arch.NUM_CLASSES, nk: int = arch.NUM_KPT_CH, net: int = 96) -> dict:
    """-> state-dict {name: fp32 array}.  (Computed once per argument set; every call gets its own copy.)"""
    return {k: v.copy() for k, v in _cached(seed, nc, nk, net).items()}


@functools.lru_cache(maxsize=2)
def imported_blob(seed: int = 0, report: bool = False):
    """The checkpoint the way a user brings it: folded, written as an fp32 export with the network's node list by a real
    protobuf serializer, and imported.  -> the .irmw blob (with report=True: (blob, the importer's report))."""
    import onnx_files
    from irmv_detection_amd import onnx_import
    rep = []
    blob = onnx_import.convert(onnx_files.write_model(fold(make(seed)), "raw32", nodes="ultralytics"), rep)
    return (blob, rep) if report else blob


def fp16_ties(x32: np.ndarray) -> np.ndarray:
    """Which fp32 values lie exactly half way between two neighbouring fp16 values (subnormal spacing below 2^-14)."""
    a = np.abs(np.asarray(x32, np.float32)).astype(np.float64)
    _, e = np.frexp(a)                                        # a = m 2^e, m in [0.5, 1)
    ulp = np.exp2(np.maximum(e - 1, -14) - 10.0)
    t = a / ulp                                               # exact: a power of two divides
    return (a > 0) & (a < 65520.0) & (t - np.floor(t) == 0.5)


def _int8_layers(blob: bytes):
    """[(ConvSpec, offset of the int8 weights, offset of the fp32 scales)] of an int8 blob."""
    import struct
    _, layers = weights.parse_blob(blob)
    out = []
    for i, (sp, _, _) in enumerate(layers):
        w_off = struct.unpack_from(weights.LAYER_FMT, blob, weights.HEADER_SIZE + i * weights.LAYER_SIZE)[7]
        out.append((sp, w_off, w_off + (sp.n_weights + 3) // 4 * 4))
    return out


def int8_blob_with_ties(seed: int = 0):
    """The imported checkpoint quantised to int8, with one dead channel of model.6.cv1 (one whose bias is 0, so that its
    output is as small as its weights make it) rewritten by hand: scale = 2^-25 and every q odd, so every q * scale is an
    odd number of half steps of 2^-24 -- an fp16 subnormal on a rounding tie (q = 1 -> 0, 3 -> 2 steps, 5 -> 2, 7 -> 4, ...).
    -> (blob, layer, channel)"""
    blob = bytearray(weights.quantize_blob_int8(imported_blob(seed)))
    _, layers = weights.parse_blob(bytes(blob))
    sp, w_off, s_off = next(l for l in _int8_layers(bytes(blob)) if l[0].name == "model.6.cv1")
    w, b = next((w, b) for spec, w, b in layers if spec.name == sp.name)
    c = int(np.flatnonzero(~w.reshape(sp.cout, -1).any(axis=1) & (b == 0))[0])
    per_out = sp.cin * sp.k * sp.k
    q = (2 * ((np.arange(per_out) * 37) % 127) - 125).astype(np.int8)          # odd values in [-125, 127]
    assert (q % 2 != 0).all() and q.max() == 127
    blob[w_off + c * per_out:w_off + (c + 1) * per_out] = q.tobytes()
    blob[s_off + 4 * c:s_off + 4 * c + 4] = np.float32(2.0 ** -25).tobytes()
    return bytes(blob), sp.name, c


def int8_products(blob: bytes):
    """Over every q * scale (fp32) of an int8 blob -> (how many are fp16 subnormals, how many lie on an fp16 rounding tie,
    how many are both)."""
    n_sub = n_tie = n_both = 0
    for sp, w_off, s_off in _int8_layers(blob):
        q = np.frombuffer(blob, np.int8, sp.n_weights, w_off).reshape(sp.cout, -1).astype(np.float32)
        x = q * np.frombuffer(blob, np.float32, sp.cout, s_off)[:, None]
        sub = (x != 0) & (np.abs(x) < 2.0 ** -14)
        tie = fp16_ties(x)
        n_sub, n_tie, n_both = n_sub + int(sub.sum()), n_tie + int(tie.sum()), n_both + int((sub & tie).sum())
    return n_sub, n_tie, n_both


def fold(ckpt: dict) -> dict:
    """BatchNorm fusion in float64: w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps).
    -> {<stem>.weight (OIHW), <stem>.bias}, the names a fused export carries."""
    out = {}
    for key in ckpt:
        if key.endswith(".bn.weight"):
            m = key[:-len(".bn.weight")]
            g = ckpt[key].astype(np.float64) / np.sqrt(ckpt[m + ".bn.running_var"].astype(np.float64) + EPS)
            out[m + ".conv.weight"] = ckpt[m + ".conv.weight"].astype(np.float64) * g[:, None, None, None]
            out[m + ".conv.bias"] = ckpt[m + ".bn.bias"].astype(np.float64) - ckpt[m + ".bn.running_mean"].astype(np.float64) * g
        elif ".bn." not in key and not key.endswith(".conv.weight"):
            out[key] = ckpt[key].astype(np.float64)
    return out


def expected_tensors(src: dict, stored_dtype, specs=None):
    """What the blob must hold for `src` (a checkpoint, folded here, or a dict of fused convs) exported in `stored_dtype`:
    the value rounded to the file's dtype, then ONE round-to-nearest-even to fp16 for weights (NumPy's direct cast) and to
    fp32 for biases.  -> [(w fp16 OHWI, b fp32)] in the order of `specs` (default: the layer table the head sizes give)."""
    fused = fold(src) if any(".bn." in k for k in src) else src
    if specs is None:
        nk = fused["model.22.cv4.0.2.weight"].shape[0] if "model.22.cv4.0.2.weight" in fused else 0
        backbone = arch.BACKBONE_SHUFFLE if "model.2.b1.dw.conv.weight" in fused else arch.BACKBONE_C2F
        specs = arch.conv_specs(fused["model.22.cv3.0.2.weight"].shape[0], nk, backbone)
    out = []
    for sp in specs:
        w = np.asarray(fused[stem(sp) + ".weight"]).astype(stored_dtype)
        b = np.asarray(fused[stem(sp) + ".bias"]).astype(stored_dtype)
        out.append((np.ascontiguousarray(w.astype(np.float16).transpose(0, 2, 3, 1)), np.ascontiguousarray(b.astype(np.float32))))
    return out
