"""ONNX files written by a real protobuf serializer, for tests/test_onnx_files.py and tests/test_checkpoint.py.

Test infrastructure.  The importer (irmv_detection_amd/onnx_import.py) reads protobuf by hand and, before this module, had
only met files from its own writer.  Here the message classes are built at import time with google.protobuf from the field
numbers of the public ONNX schema (onnx.proto: TensorProto, NodeProto, AttributeProto, GraphProto, ModelProto, ...), proto2
syntax, and the files come out of SerializeToString().  No `onnx` package is involved.  A second set of classes marks
TensorProto.dims packed, which is what a proto3-style writer emits.

    write_model(tensors, encoding, nodes=None, extras=True, order=None) -> bytes

`tensors` is {initializer name: array}: the fused convs under their Ultralytics names, weights OIHW (named() makes it from a
layer table).  `encoding` chooses the stored dtype and the TensorProto field that carries it (ENCODINGS).
"""
from __future__ import annotations

import numpy as np
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

from irmv_detection_amd import arch

_F = descriptor_pb2.FieldDescriptorProto
_OPT, _REP = _F.LABEL_OPTIONAL, _F.LABEL_REPEATED

# TensorProto.DataType / AttributeProto.AttributeType of the ONNX schema
FLOAT, INT64, FLOAT16, DOUBLE, BFLOAT16 = 1, 7, 10, 11, 16
A_FLOAT, A_INT, A_STRING, A_TENSOR, A_INTS = 1, 2, 3, 4, 7


def _classes(package: str, dims_packed: bool):
    fd = descriptor_pb2.FileDescriptorProto(name=package + ".proto", package=package, syntax="proto2")

    def message(name, *fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, extra in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if isinstance(extra, str):
                f.type_name = f".{package}.{extra}"
            elif extra:
                f.options.packed = True

    message("StringStringEntryProto", ("key", 1, _F.TYPE_STRING, _OPT, None), ("value", 2, _F.TYPE_STRING, _OPT, None))
    message("OperatorSetIdProto", ("domain", 1, _F.TYPE_STRING, _OPT, None), ("version", 2, _F.TYPE_INT64, _OPT, None))
    message("ValueInfoProto", ("name", 1, _F.TYPE_STRING, _OPT, None))
    message("TensorProto",
            ("dims", 1, _F.TYPE_INT64, _REP, dims_packed), ("data_type", 2, _F.TYPE_INT32, _OPT, None),
            ("float_data", 4, _F.TYPE_FLOAT, _REP, True), ("int32_data", 5, _F.TYPE_INT32, _REP, True),
            ("name", 8, _F.TYPE_STRING, _OPT, None), ("raw_data", 9, _F.TYPE_BYTES, _OPT, None),
            ("double_data", 10, _F.TYPE_DOUBLE, _REP, True), ("doc_string", 12, _F.TYPE_STRING, _OPT, None),
            ("external_data", 13, _F.TYPE_MESSAGE, _REP, "StringStringEntryProto"), ("data_location", 14, _F.TYPE_INT32, _OPT, None))
    message("AttributeProto",
            ("name", 1, _F.TYPE_STRING, _OPT, None), ("f", 2, _F.TYPE_FLOAT, _OPT, None), ("i", 3, _F.TYPE_INT64, _OPT, None),
            ("s", 4, _F.TYPE_BYTES, _OPT, None), ("t", 5, _F.TYPE_MESSAGE, _OPT, "TensorProto"),
            ("ints", 8, _F.TYPE_INT64, _REP, None), ("type", 20, _F.TYPE_INT32, _OPT, None))
    message("NodeProto",
            ("input", 1, _F.TYPE_STRING, _REP, None), ("output", 2, _F.TYPE_STRING, _REP, None), ("name", 3, _F.TYPE_STRING, _OPT, None),
            ("op_type", 4, _F.TYPE_STRING, _OPT, None), ("attribute", 5, _F.TYPE_MESSAGE, _REP, "AttributeProto"))
    message("GraphProto",
            ("node", 1, _F.TYPE_MESSAGE, _REP, "NodeProto"), ("name", 2, _F.TYPE_STRING, _OPT, None),
            ("initializer", 5, _F.TYPE_MESSAGE, _REP, "TensorProto"), ("input", 11, _F.TYPE_MESSAGE, _REP, "ValueInfoProto"),
            ("output", 12, _F.TYPE_MESSAGE, _REP, "ValueInfoProto"), ("value_info", 13, _F.TYPE_MESSAGE, _REP, "ValueInfoProto"))
    message("ModelProto",
            ("ir_version", 1, _F.TYPE_INT64, _OPT, None), ("producer_name", 2, _F.TYPE_STRING, _OPT, None),
            ("graph", 7, _F.TYPE_MESSAGE, _OPT, "GraphProto"), ("opset_import", 8, _F.TYPE_MESSAGE, _REP, "OperatorSetIdProto"),
            ("metadata_props", 14, _F.TYPE_MESSAGE, _REP, "StringStringEntryProto"))
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return {m.name: message_factory.GetMessageClass(pool.FindMessageTypeByName(f"{package}.{m.name}")) for m in fd.message_type}


PB = _classes("onnx_proto2", False)
PB_DIMS_PACKED = _classes("onnx_dims_packed", True)

# encoding -> (stored dtype, TensorProto field that carries the values)
ENCODINGS = {
    "raw32": (np.float32, "raw_data"),
    "float_data": (np.float32, "float_data"),
    "raw16": (np.float16, "raw_data"),           # fp16 weights and fp16 biases: an Ultralytics half=True export
    "int32_fp16": (np.float16, "int32_data"),    # how ONNX stores fp16 outside raw_data: the bits, one per int32
    "raw64": (np.float64, "raw_data"),
    "double_data": (np.float64, "double_data"),
    "dims_packed": (np.float32, "raw_data"),
}
_ONNX_TYPE = {np.dtype(np.float32): FLOAT, np.dtype(np.float16): FLOAT16, np.dtype(np.float64): DOUBLE}


def stored_dtype(encoding: str):
    return ENCODINGS[encoding][0]


def stem(sp: arch.ConvSpec) -> str:
    """Initializer stem of a layer: Ultralytics Conv modules keep their conv under `.conv`, the Detect finals are plain Conv2d."""
    final = sp.name.startswith("model.22.") and sp.name.endswith(".2")
    return sp.name if (final or sp.name.endswith(".conv")) else sp.name + ".conv"


def named(specs, tensors) -> dict:
    """A layer table's (w OHWI, b) pairs -> {initializer name: array}, weights OIHW."""
    out = {}
    for sp, (w, b) in zip(specs, tensors):
        out[stem(sp) + ".weight"] = np.ascontiguousarray(np.asarray(w).transpose(0, 3, 1, 2))
        out[stem(sp) + ".bias"] = np.asarray(b)
    return out


def tensor_proto(pb, name: str, arr, encoding: str = "raw32", onnx_type=None):
    """One TensorProto.  An integer array goes in as an int64 constant (raw_data); `onnx_type` overrides data_type (the
    refusal tests label a tensor BFLOAT16 that way)."""
    t = pb["TensorProto"](name=name)
    arr = np.asarray(arr)
    t.dims.extend(int(d) for d in arr.shape)
    if arr.dtype.kind in "iu":
        t.data_type, t.raw_data = INT64, arr.astype("<i8").tobytes()
        return t
    dt, field = ENCODINGS[encoding]
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(arr.astype(dt))
    t.data_type = _ONNX_TYPE[np.dtype(dt)] if onnx_type is None else onnx_type
    if field == "raw_data":
        t.raw_data = a.astype(a.dtype.newbyteorder("<")).tobytes()
    elif field == "int32_data":
        t.int32_data.extend(a.reshape(-1).view(np.uint16).astype(np.int32).tolist())
    else:
        getattr(t, field).extend(a.reshape(-1).tolist())
    return t


def _attr(pb, name, value):
    a = pb["AttributeProto"](name=name)
    if isinstance(value, (list, tuple)):
        a.type = A_INTS
        a.ints.extend(int(v) for v in value)
    elif isinstance(value, float):
        a.type, a.f = A_FLOAT, value
    elif isinstance(value, (bytes, str)):
        a.type, a.s = A_STRING, value.encode() if isinstance(value, str) else value
    else:
        a.type, a.i = A_INT, int(value)
    return a


class _Graph:
    """Emits the node list of the network the way an Ultralytics export looks: `/model.N/.../Op_output_0` value names, Conv
    with explicit kernel_shape / strides / pads / group / dilations, SiLU as Sigmoid + Mul, shape arguments as int64
    initializers.  The topology is tests/torch_ref.py's."""

    def __init__(self, pb, specs, *, activation="silu", overrides=None):
        self.pb, self.nodes, self.consts, self.n = pb, [], {}, 0
        self.specs = {sp.name: sp for sp in specs}
        self.activation, self.overrides = activation, overrides or {}

    def node(self, op, inputs, n_out=1, scope="", **attrs):
        self.n += 1
        base = f"/{scope}/{op}_{self.n}" if scope else f"/{op}_{self.n}"
        outs = [f"{base}_output_{i}" for i in range(n_out)]
        nd = self.pb["NodeProto"](name=base, op_type=op, input=inputs, output=outs)
        nd.attribute.extend(_attr(self.pb, k, v) for k, v in attrs.items())
        self.nodes.append(nd)
        return outs[0] if n_out == 1 else outs

    def const(self, values, dtype=np.int64):
        self.n += 1
        name = f"/Constant_{self.n}_output_0"
        self.consts[name] = np.asarray(values, dtype)
        return name

    def conv(self, name, x):
        sp = self.specs[name]
        module = name[:-5] if name.endswith(".conv") else name
        a = dict(dilations=[1, 1], group=sp.groups, kernel_shape=[sp.k, sp.k], pads=[sp.k // 2] * 4, strides=[sp.stride, sp.stride])
        a.update(self.overrides.get(name, {}))
        y = self.node("Conv", [x, stem(sp) + ".weight", stem(sp) + ".bias"], scope=module + "/conv", **a)
        if sp.act != arch.ACT_SILU:
            return y
        if self.activation == "relu":
            return self.node("Relu", [y], scope=module + "/act")
        s = self.node("Sigmoid", [y], scope=module + "/act")
        return self.node("Mul", [y, s], scope=module + "/act")

    def cat(self, xs, scope=""):
        return self.node("Concat", list(xs), scope=scope, axis=1)

    def split2(self, x, c, scope=""):
        return self.node("Split", [x, self.const([c // 2, c // 2])], 2, scope=scope, axis=1)

    def up(self, x, scope):
        return self.node("Resize", [x, "", self.const([1.0, 1.0, 2.0, 2.0], np.float32)], scope=scope,
                         coordinate_transformation_mode="asymmetric", mode="nearest", nearest_mode="floor")

    def pool(self, x, scope):
        return self.node("MaxPool", [x], scope=scope, ceil_mode=0, kernel_shape=[5, 5], pads=[2, 2, 2, 2], strides=[1, 1])

    def c2f(self, prefix, x, n, shortcut):
        c = self.specs[f"{prefix}.cv1"].cout
        y = list(self.split2(self.conv(f"{prefix}.cv1", x), c, prefix))
        for i in range(n):
            t = self.conv(f"{prefix}.m.{i}.cv2", self.conv(f"{prefix}.m.{i}.cv1", y[-1]))
            y.append(self.node("Add", [y[-1], t], scope=f"{prefix}.m.{i}") if shortcut else t)
        return self.conv(f"{prefix}.cv2", self.cat(y, prefix))

    def shuffle(self, x, c, scope):
        r = self.node("Reshape", [x, self.const([0, 2, c // 2, 0, -1])], scope=scope)       # (the spatial dims stay symbolic)
        t = self.node("Transpose", [r], scope=scope, perm=[0, 2, 1, 3, 4])
        return self.node("Reshape", [t, self.const([0, c, 0, -1])], scope=scope)

    def shuffle_down(self, prefix, x):
        b1 = self.conv(f"{prefix}.b1.pw", self.conv(f"{prefix}.b1.dw", x))
        b2 = self.conv(f"{prefix}.b2.pw2", self.conv(f"{prefix}.b2.dw", self.conv(f"{prefix}.b2.pw1", x)))
        return self.shuffle(self.cat([b1, b2], prefix), 2 * self.specs[f"{prefix}.b1.pw"].cout, prefix)

    def shuffle_unit(self, prefix, x):
        c = 2 * self.specs[f"{prefix}.b2.pw1"].cout
        x1, x2 = self.split2(x, c, prefix)
        b2 = self.conv(f"{prefix}.b2.pw2", self.conv(f"{prefix}.b2.dw", self.conv(f"{prefix}.b2.pw1", x2)))
        return self.shuffle(self.cat([x1, b2], prefix), c, prefix)

    def network(self, nk, backbone):
        a1 = self.conv("model.1.conv", self.conv("model.0.conv", "images"))
        if backbone == arch.BACKBONE_SHUFFLE:
            a4 = self.shuffle_unit("model.3", self.shuffle_down("model.2", a1))
            a6 = self.shuffle_unit("model.6", self.shuffle_unit("model.5", self.shuffle_down("model.4", a4)))
            a8 = self.shuffle_unit("model.8", self.shuffle_down("model.7", a6))
        else:
            a4 = self.c2f("model.4", self.conv("model.3.conv", self.c2f("model.2", a1, 1, True)), 2, True)
            a6 = self.c2f("model.6", self.conv("model.5.conv", a4), 2, True)
            a8 = self.c2f("model.8", self.conv("model.7.conv", a6), 1, True)
        a = self.conv("model.9.cv1", a8)
        p1 = self.pool(a, "model.9/m")
        p2 = self.pool(p1, "model.9/m")
        p3 = self.pool(p2, "model.9/m")
        a9 = self.conv("model.9.cv2", self.cat([a, p1, p2, p3], "model.9"))
        a12 = self.c2f("model.12", self.cat([self.up(a9, "model.10"), a6], "model.11"), 1, False)
        a15 = self.c2f("model.15", self.cat([self.up(a12, "model.13"), a4], "model.14"), 1, False)
        a18 = self.c2f("model.18", self.cat([self.conv("model.16.conv", a15), a12], "model.17"), 1, False)
        a21 = self.c2f("model.21", self.cat([self.conv("model.19.conv", a18), a9], "model.20"), 1, False)
        outs = []
        for i, p in enumerate((a15, a18, a21)):
            br = []
            for b in ("cv2", "cv3") + (("cv4",) if nk > 0 else ()):
                h = self.conv(f"model.22.{b}.{i}.1", self.conv(f"model.22.{b}.{i}.0", p))
                br.append(self.conv(f"model.22.{b}.{i}.2", h))
            o = self.cat(br, "model.22")
            no = self.specs[f"model.22.cv2.{i}.2"].cout + self.specs[f"model.22.cv3.{i}.2"].cout + max(nk, 0)
            outs.append(self.node("Reshape", [o, self.const([1, no, -1])], scope="model.22"))
        return self.node("Concat", outs, scope="model.22", axis=2)


def write_model(tensors: dict, encoding: str = "raw32", *, nodes=None, extras: bool = True, order=None,
                activation: str = "silu", overrides=None, replace=None, opset: int = 17) -> bytes:
    """A ModelProto with `tensors` as initializers, serialized by google.protobuf.

    nodes       None: initializers only.  "ultralytics": the network's node list (needs the full layer set in `tensors`).
    extras      what a real export carries besides: int64 shape constants among the initializers, the initializers listed
                again as graph inputs, doc strings, metadata props, the fixed model.22.dfl.conv.weight.
    order       a seed: shuffles the initializers.
    activation, overrides    (test knobs for nodes) "relu" writes a ReLU export; overrides = {layer: {attribute: value}}.
    replace     {initializer name: TensorProto or None}: swap in a hand-made tensor, or drop one.
    """
    pb = PB_DIMS_PACKED if encoding == "dims_packed" else PB
    model = pb["ModelProto"](ir_version=8, producer_name="pytorch")
    g = model.graph
    g.name = "main_graph"
    consts = {}
    if nodes == "ultralytics":
        nc = tensors["model.22.cv3.0.2.weight"].shape[0]
        nk = tensors["model.22.cv4.0.2.weight"].shape[0] if "model.22.cv4.0.2.weight" in tensors else 0
        backbone = arch.BACKBONE_SHUFFLE if "model.2.b1.dw.conv.weight" in tensors else arch.BACKBONE_C2F
        gr = _Graph(pb, arch.conv_specs(nc, nk, backbone), activation=activation, overrides=overrides)
        out = gr.network(nk, backbone)
        g.node.extend(gr.nodes)
        g.output.add(name=out)
        consts = gr.consts
    elif nodes is not None:
        raise ValueError(nodes)
    items = list(tensors.items())
    if extras:
        items.append(("model.22.dfl.conv.weight", np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)))
        consts = dict(consts)
        consts["/model.22/Constant_output_0"] = np.array([1, 4, 16, -1], np.int64)
        consts["/model.22/Constant_1_output_0"] = np.array([0.5], np.float32)
    items += list(consts.items())
    if order is not None:
        perm = np.random.default_rng(order).permutation(len(items))
        items = [items[i] for i in perm]
    g.input.add(name="images")
    for name, arr in items:
        if replace and name in replace:
            if replace[name] is None:
                continue
            t = replace[name]
        else:
            t = tensor_proto(pb, name, arr, encoding if name in tensors else "raw32")
        if extras and name in tensors and name.endswith(".weight"):
            t.doc_string = "fused conv weight of " + name[:-7]
        g.initializer.append(t)
        if extras:
            g.input.add(name=name)          # exports with keep_initializers_as_inputs list every initializer again
    model.opset_import.add(domain="", version=opset)
    if extras:
        for k, v in (("author", "Ultralytics"), ("task", "pose"), ("stride", "32"), ("imgsz", "[640, 640]"),
                     ("names", "{0: 'B1', 1: 'B2'}")):
            model.metadata_props.add(key=k, value=v)
    return model.SerializeToString()
