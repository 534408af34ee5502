"""ONNX -> .irmw converter.

The reference's on-disk model is a TensorRT engine built from `models/yolov7.onnx`
with trtexec (reference src/yolo_engine.cpp:28-40, README.md).  This build's
engine loads `<stem>.irmw` instead; this module produces it from the same ONNX
file.  No `onnx` package exists in the image, so the few protobuf fields needed
are decoded by hand (ModelProto.graph = 7; GraphProto.node = 1, initializer = 5;
TensorProto: dims = 1, data_type = 2, float_data = 4, int32_data = 5, name = 8, raw_data = 9,
double_data = 10, external_data = 13, data_location = 14; NodeProto: input = 1, output = 2,
name = 3, op_type = 4, attribute = 5; AttributeProto: name = 1, f = 2, i = 3, ints = 8).

Expected input: an Ultralytics YOLOv8n / YOLOv8n-pose export (BatchNorm already
folded into the convs, so every conv initializer pair is `<layer>.weight`,
`<layer>.bias`, OIHW; fp32, fp16 or fp64, in raw_data or the typed field).  Layer names must be the Ultralytics ones
listed by `arch.conv_specs` (`model.0.conv`, `model.2.m.0.cv1.conv`, ...,
`model.22.cv2.0.2`); the fixed DFL conv (`model.22.dfl.conv`) is ignored.  Values are
rounded to fp16 once, from the dtype the file stores.  The file is refused, with a message
that names the layer, when it holds a NaN / Inf or a weight that overflows fp16, keeps its
data outside the file, still carries BatchNorm, or when its graph (if it has nodes) disagrees
with the layer table on a conv's geometry or activation ("ONNX files").

    python -m irmv_detection_amd.onnx_import models/yolov7.onnx      # writes models/yolov7.irmw
"""
from __future__ import annotations

import struct
import sys
from typing import Dict, Optional, Tuple

import numpy as np

from . import arch, weights


def _varint(buf: bytes, pos: int) -> Tuple[int, int]:
    out = shift = 0
    n = len(buf)
    while True:
        if pos >= n:
            raise ValueError("truncated protobuf: a varint runs past the end of its buffer")
        if shift > 63:
            raise ValueError("malformed protobuf: a varint longer than 10 bytes")
        b = buf[pos]
        pos += 1
        out |= (b & 0x7F) << shift
        if not b & 0x80:
            return out, pos
        shift += 7


def _fields(buf: bytes):
    """Yield (field number, wire type, value) of one protobuf message.  A field that runs past the end of `buf` (a file
    cut short, at any nesting: every nested message is parsed from the slice its parent handed out) is a ValueError."""
    pos, n = 0, len(buf)
    while pos < n:
        key, pos = _varint(buf, pos)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
            yield fno, wt, val
            continue
        if wt == 1:
            ln = 8
        elif wt == 2:
            ln, pos = _varint(buf, pos)
        elif wt == 5:
            ln = 4
        else:
            raise ValueError(f"unsupported protobuf wire type {wt}")
        if pos + ln > n:
            raise ValueError(f"truncated protobuf: field {fno} needs {ln} bytes, {n - pos} are left in its buffer")
        yield fno, wt, buf[pos:pos + ln]
        pos += ln


def _varints(buf: bytes) -> np.ndarray:
    """Every varint of a packed field at once -> uint64 array."""
    b = np.frombuffer(buf, np.uint8)
    if not len(b):
        return np.zeros(0, np.uint64)
    last = b < 0x80
    if not last[-1]:
        raise ValueError("truncated protobuf: a packed varint runs past the end of its field")
    starts = np.concatenate(([0], np.flatnonzero(last)[:-1] + 1))
    k = np.arange(len(b)) - np.repeat(starts, np.diff(np.concatenate((starts, [len(b)]))))
    if k.max() > 9:
        raise ValueError("malformed protobuf: a varint longer than 10 bytes")
    return np.add.reduceat((b & 0x7F).astype(np.uint64) << (7 * k).astype(np.uint64), starts)


# TensorProto.data_type values (public ONNX schema); the three this importer reads, and names for the refusal of the rest
_DTYPES = {1: np.float32, 10: np.float16, 11: np.float64}
_DTYPE_NAMES = {0: "UNDEFINED", 1: "FLOAT", 2: "UINT8", 3: "INT8", 4: "UINT16", 5: "INT16", 6: "INT32", 7: "INT64", 8: "STRING",
                9: "BOOL", 10: "FLOAT16", 11: "DOUBLE", 12: "UINT32", 13: "UINT64", 14: "COMPLEX64", 15: "COMPLEX128",
                16: "BFLOAT16", 17: "FLOAT8E4M3FN", 18: "FLOAT8E4M3FNUZ", 19: "FLOAT8E5M2", 20: "FLOAT8E5M2FNUZ"}


class _Tensor:
    """One TensorProto as the file states it; nothing is checked until `array()` is asked for."""
    __slots__ = ("name", "dims", "dtype", "raw", "floats", "ints", "doubles", "external")

    def __init__(self, buf: bytes):
        self.name, self.dims, self.dtype, self.raw = "", [], 1, None
        self.floats, self.ints, self.doubles, self.external = [], [], [], False
        for fno, wt, val in _fields(buf):
            if fno == 1:
                self.dims += [val] if wt == 0 else [int(d) for d in _varints(val)]      # (packed by proto3-style writers)
            elif fno == 2:
                self.dtype = val
            elif fno == 8:
                self.name = val.decode()
            elif fno == 9:
                self.raw = val
            elif fno == 4:       # float_data: packed (wire type 2) or one fixed32 per element
                self.floats.append(val)
            elif fno == 5:       # int32_data: packed varints or one varint per element; fp16 tensors keep their bits here
                self.ints.append(_varints(val) if wt == 2 else np.array([val], np.uint64))
            elif fno == 10:      # double_data: packed or one fixed64 per element
                self.doubles.append(val)
            elif fno == 13 or (fno == 14 and val == 1):
                self.external = True

    def array(self) -> np.ndarray:
        """The stored values in the stored dtype, shaped by dims.  ValueError names the tensor and what is wrong."""
        if self.external:
            raise ValueError(f"{self.name}: the tensor's data is external (data_location = EXTERNAL / external_data); "
                             f"export the model as one self-contained file")
        if self.dtype not in _DTYPES:
            raise ValueError(f"{self.name}: unsupported data_type {self.dtype} ({_DTYPE_NAMES.get(self.dtype, '?')}); "
                             f"FLOAT, FLOAT16 and DOUBLE are read")
        dt = np.dtype(_DTYPES[self.dtype])
        count = int(np.prod(self.dims, dtype=np.int64)) if self.dims else 1
        if self.raw is not None:
            if len(self.raw) != count * dt.itemsize:
                raise ValueError(f"{self.name}: raw_data holds {len(self.raw)} bytes, dims {self.dims} of "
                                 f"{_DTYPE_NAMES[self.dtype]} need {count * dt.itemsize}")
            arr = np.frombuffer(self.raw, dt.newbyteorder("<"))
        elif self.dtype == 1 and self.floats:
            arr = np.frombuffer(b"".join(self.floats), "<f4")
        elif self.dtype == 10 and self.ints:
            arr = np.concatenate(self.ints).astype(np.uint16).view(np.float16)      # the low 16 bits of each int32
        elif self.dtype == 11 and self.doubles:
            arr = np.frombuffer(b"".join(self.doubles), "<f8")
        else:
            raise ValueError(f"{self.name}: no payload for {_DTYPE_NAMES[self.dtype]} (raw_data or the typed field of that type)")
        if arr.size != count:
            raise ValueError(f"{self.name}: payload holds {arr.size} elements, dims {self.dims} need {count}")
        return arr.reshape(self.dims) if self.dims else arr


class _Node:
    __slots__ = ("inputs", "outputs", "name", "op", "attrs")

    def __init__(self, buf: bytes):
        self.inputs, self.outputs, self.name, self.op, self.attrs = [], [], "", "", {}
        for fno, wt, val in _fields(buf):
            if fno == 1:
                self.inputs.append(val.decode())
            elif fno == 2:
                self.outputs.append(val.decode())
            elif fno == 3:
                self.name = val.decode()
            elif fno == 4:
                self.op = val.decode()
            elif fno == 5 and wt == 2:      # AttributeProto: name = 1, i = 3, ints = 8 (the integer attributes are all a Conv has)
                an, ai, ais = "", None, []
                for f2, w2, v2 in _fields(val):
                    if f2 == 1:
                        an = v2.decode()
                    elif f2 == 3 and w2 == 0:
                        ai = v2
                    elif f2 == 2 and w2 == 5 and ai is None:      # f: a Gemm's alpha / beta (number_net.py)
                        ai = struct.unpack("<f", v2)[0]
                    elif f2 == 8:
                        ais += [v2] if w2 == 0 else [int(d) for d in _varints(v2)]
                self.attrs[an] = ais if ais else ai


def _read_graph(onnx_bytes: bytes):
    """-> ({initializer name: _Tensor}, [_Node])"""
    graph = None
    for fno, wt, val in _fields(onnx_bytes):
        if fno == 7 and wt == 2:
            graph = val
    if graph is None:
        raise ValueError("no GraphProto in the ONNX file")
    init, nodes = {}, []
    for fno, wt, val in _fields(graph):
        if fno == 5 and wt == 2:
            t = _Tensor(val)
            init[t.name] = t
        elif fno == 1 and wt == 2:
            nodes.append(_Node(val))
    return init, nodes


def read_initializers(onnx_bytes: bytes) -> Dict[str, np.ndarray]:
    """Every initializer this importer can read (FLOAT, FLOAT16, DOUBLE, data in the file), in its stored dtype."""
    out = {}
    for name, t in _read_graph(onnx_bytes)[0].items():
        if not t.external and t.dtype in _DTYPES:
            out[name] = t.array()
    return out


def _lookup(init: Dict[str, "_Tensor"], layer: str):
    """Ultralytics names: Conv modules keep their conv under `.conv`; the head's plain Conv2d do not.
    -> (weight name, weight, bias), all None when the layer has no weight initializer."""
    for stem in (layer, layer + ".conv", layer.replace(".conv", "") + ".conv"):
        w = init.get(stem + ".weight")
        if w is not None:
            b = init.get(stem + ".bias")
            if b is None:
                raise ValueError(f"{layer}: {stem}.weight has no {stem}.bias beside it (a conv exported without its bias: "
                                 f"BatchNorm not fused, or bias=False)")
            return stem + ".weight", w.array(), b.array()
    return None, None, None


def _check_node(sp: arch.ConvSpec, wname: str, nodes) -> None:
    """The graph around one layer's weight: the Conv's geometry is the layer table's, and SiLU (Sigmoid + Mul) follows it
    exactly where the table says act == 1."""
    convs = [n for n in nodes if n.op == "Conv" and wname in n.inputs[1:2]]
    if len(convs) != 1:
        raise ValueError(f"{sp.name}: {len(convs)} Conv nodes consume {wname}, one is expected")
    n = convs[0]
    got = dict(kernel_shape=n.attrs.get("kernel_shape") or [sp.k, sp.k], strides=n.attrs.get("strides") or [1, 1],
               pads=n.attrs.get("pads") or [0, 0, 0, 0], group=n.attrs.get("group") or 1,
               dilations=n.attrs.get("dilations") or [1, 1])
    if n.attrs.get("auto_pad") is not None:
        raise ValueError(f"{sp.name}: Conv uses auto_pad; explicit pads = {sp.k // 2} are expected")
    want = dict(kernel_shape=[sp.k, sp.k], strides=[sp.stride, sp.stride], pads=[sp.k // 2] * 4, group=sp.groups, dilations=[1, 1])
    for key, v in want.items():
        if got[key] != v:
            raise ValueError(f"{sp.name}: Conv {key} = {got[key]} in the file, the layer table says {v}")
    users = [m for m in nodes if n.outputs and n.outputs[0] in m.inputs]
    sig = [m for m in users if m.op == "Sigmoid"]
    if sp.act == arch.ACT_SILU:
        mul = [m for m in users if m.op == "Mul" and sig and sig[0].outputs[0] in m.inputs]
        if len(sig) != 1 or len(mul) != 1:
            raise ValueError(f"{sp.name}: the Conv is followed by {sorted(m.op for m in users)}, not by SiLU (Sigmoid + Mul): "
                             f"this engine computes SiLU after this layer")
    elif sig:
        raise ValueError(f"{sp.name}: the Conv feeds a Sigmoid, but this engine applies no activation after this layer")


def _channel_of(mask: np.ndarray) -> int:
    return int(np.flatnonzero(mask.reshape(mask.shape[0], -1).any(axis=1))[0])


def convert(onnx_bytes: bytes, report: Optional[list] = None) -> bytes:
    """ONNX file -> .irmw blob.  `report`, when a list, gets one tuple per layer appended: (layer, weights that are not
    zero in the file and zero in fp16, weights that land in the fp16 subnormal range and lose bits there, max |w| of the
    file).  Both counts are of weights the rounding changed: a stored value that is an fp16 subnormal exactly (a file made
    from fp16 weights has some) lost nothing and is not counted."""
    init, nodes = _read_graph(onnx_bytes)
    bn = sorted(n for n in init if ".bn." in n) or sorted(n.name or n.op for n in nodes if n.op == "BatchNormalization")
    if bn:
        raise ValueError(f"the file still carries BatchNorm ({bn[0]}, {len(bn)} in all): export with fused BatchNorm")
    # head sizes from the final convs of level 0
    _, wc, _ = _lookup(init, "model.22.cv3.0.2")
    if wc is None:
        raise ValueError("model.22.cv3.0.2 not found: not an Ultralytics YOLOv8 detect/pose export")
    nc = int(wc.shape[0]) if wc.ndim else 0
    _, wk, _ = _lookup(init, "model.22.cv4.0.2")
    nk = int(wk.shape[0]) if wk is not None and wk.ndim else 0
    if nk not in (0, 8):
        raise ValueError(f"keypoint head has {nk} outputs; this engine supports 4 keypoints x (x, y) = 8")
    # the ShuffleNetV2-backbone variant (arch.BACKBONE_SHUFFLE) is recognised by its first depthwise conv; its layer names
    # are this build's (the external repository the reference's README points to is not available offline)
    shuffle = any(("model.2.b1.dw" + s) in init for s in (".weight", ".conv.weight"))
    backbone = arch.BACKBONE_SHUFFLE if shuffle else arch.BACKBONE_C2F
    specs = arch.conv_specs(nc, nk, backbone)
    tensors = []
    for sp in specs:
        wname, w, b = _lookup(init, sp.name)
        if w is None:
            raise ValueError(f"initializers of {sp.name} not found")
        if tuple(w.shape) != (sp.cout, sp.cin, sp.k, sp.k) or b.shape != (sp.cout,):
            raise ValueError(f"{sp.name}: shape {tuple(w.shape)} does not match the layer table ({sp.cout}, {sp.cin}, {sp.k}, {sp.k})")
        if not np.isfinite(w).all():
            raise ValueError(f"{sp.name}: output channel {_channel_of(~np.isfinite(w))} holds a NaN or Inf weight")
        with np.errstate(over="ignore"):
            w16 = w.astype(np.float16)          # ONE rounding, straight from the stored dtype (never fp64 -> fp32 -> fp16)
            b32 = b.astype(np.float32)
        if np.isinf(w16).any():
            o = _channel_of(np.isinf(w16))
            raise ValueError(f"{sp.name}: output channel {o} holds a weight of magnitude {float(np.abs(w[o]).max()):g}, which "
                             f"rounds to an fp16 infinity (|w| >= 65520)")
        if not np.isfinite(b32).all():
            raise ValueError(f"{sp.name}: the bias of output channel {int(np.flatnonzero(~np.isfinite(b32))[0])} is not finite")
        if nodes:
            _check_node(sp, wname, nodes)
        if report is not None:
            a16 = np.abs(w16)
            report.append((sp.name, int(((w != 0) & (w16 == 0)).sum()), int(((a16 > 0) & (a16 < 2.0 ** -14) & (w16 != w)).sum()),
                           float(np.abs(w).max())))
        tensors.append((np.ascontiguousarray(w16.transpose(0, 2, 3, 1)), np.ascontiguousarray(b32)))       # OIHW -> OHWI
    return weights.build_blob(specs, tensors, nc, nk, backbone)


# ---- minimal writer, used by the tests to make an ONNX file to import -------------
def _enc_varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _enc_field(fno: int, payload: bytes) -> bytes:
    return _enc_varint((fno << 3) | 2) + _enc_varint(len(payload)) + payload


def write_initializer_only_onnx(tensors: Dict[str, np.ndarray]) -> bytes:
    """An ONNX ModelProto that carries nothing but named fp32 initializers."""
    graph = b""
    for name, arr in tensors.items():
        arr = np.ascontiguousarray(arr, np.float32)
        t = b"".join(_enc_varint((1 << 3) | 0) + _enc_varint(int(d)) for d in arr.shape)
        t += _enc_varint((2 << 3) | 0) + _enc_varint(1)
        t += _enc_field(8, name.encode()) + _enc_field(9, arr.tobytes())
        graph += _enc_field(5, t)
    return _enc_varint((1 << 3) | 0) + _enc_varint(8) + _enc_field(7, graph)


def main(argv):
    args = [a for a in argv[1:] if a != "--int8"]
    if len(args) != 1:
        print(__doc__)
        return 2
    src = args[0]
    report = []
    with open(src, "rb") as f:
        blob = convert(f.read(), report)
    for layer, n_zero, n_sub, amax in report:
        if n_zero or n_sub:
            print(f"{layer}: {n_zero} weights round to zero in fp16, {n_sub} are rounded to fp16 subnormals (max |w| {amax:.3g})")
    if "--int8" in argv:      # per-output-channel int8 weights (BASELINE configs[4]); biases stay fp32
        blob = weights.quantize_blob_int8(blob)
    dst = weights.model_blob_path(src)
    with open(dst, "wb") as f:
        f.write(blob)
    print(f"wrote {dst} ({len(blob)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
