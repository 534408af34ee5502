"""Plate numbers on the host (include/irmv_hip.h, "plate numbers"; csrc/k_number.hip): the model object, the reference the
kernel is tested against, the .irmn model file and the ONNX import of a small MLP.

`NumberModel.reference` is the kernel's arithmetic in NumPy float32, operation for operation (NumPy fuses nothing and keeps
denormals): a unit has four chains, chain q takes the inputs k = q (mod 4) in ascending k, a_0 starts at the bias and the
others at +0, every product is rounded, then every sum, and a = (a_0 + a_1) + (a_2 + a_3).

    python -m irmv_detection_amd.number_net in.onnx out.irmn      # converts a file
"""
from __future__ import annotations

import struct
import sys
from typing import List, Optional, Sequence

import numpy as np

N_IN, HIDDEN_MAX, CLASSES_MAX, LAYERS_MAX = 560, 128, 16, 3
VALUE_MAX = 65504.0
IN_BINARY, IN_GRAY = 0, 1
_INPUTS = {"binary": IN_BINARY, "gray": IN_GRAY, IN_BINARY: IN_BINARY, IN_GRAY: IN_GRAY}
MAGIC, VERSION, HEADER_BYTES = b"IRMN", 1, 32

# irmv_plate_number, 96 bytes
NUMBER_DTYPE = np.dtype([("state", "<i4"), ("label", "<i4"), ("second", "<i4"), ("ones", "<i4"), ("margin", "<f4"),
                         ("reserved", "<i4", (3,)), ("logits", "<f4", (CLASSES_MAX,))])
assert NUMBER_DTYPE.itemsize == 96


def check_shape(dims: Sequence[int], input_mode: int) -> None:
    """ValueError where the library answers IRMV_ERR_ARG to a model's shape."""
    n = len(dims) - 1
    if not 1 <= n <= LAYERS_MAX:
        raise ValueError("a number model has 1 .. 3 layers")
    if dims[0] != N_IN:
        raise ValueError(f"the first layer must take the 560 patch values, not {dims[0]}")
    if any(not 1 <= d <= HIDDEN_MAX for d in dims[1:-1]):
        raise ValueError("a hidden width must be 1 .. 128")
    if not 1 <= dims[-1] <= CLASSES_MAX:
        raise ValueError("the last width must be 1 .. 16")
    if input_mode not in (IN_BINARY, IN_GRAY):
        raise ValueError("input must be 'binary' or 'gray'")


def patch_arrays(patches):
    """(gray uint8 [n, 560], state int64 [n], otsu int64 [n]) of patch records: capi.PlatePatch structures, the dicts of
    patches.patch, or such a triple itself."""
    if isinstance(patches, tuple) and len(patches) == 3 and isinstance(patches[0], np.ndarray):
        g, s, o = patches
        return np.ascontiguousarray(g, np.uint8).reshape(-1, N_IN), np.asarray(s, np.int64).reshape(-1), np.asarray(o, np.int64).reshape(-1)
    n = len(patches)
    gray, state, otsu = np.zeros((n, N_IN), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, p in enumerate(patches):
        if isinstance(p, dict):
            gray[i], state[i], otsu[i] = np.asarray(p["gray"], np.uint8).reshape(N_IN), p["state"], p["otsu"]
        else:
            gray[i], state[i], otsu[i] = np.frombuffer(bytes(p), np.uint8, N_IN), p.state, p.otsu
    return gray, state, otsu


class NumberModel:
    """weights[l]: [out][in] float32 (a torch.nn.Linear weight), biases[l]: [out] float32; input 'binary' or 'gray'.  The
    values are checked as irmv_engine_set_number_model checks them; `w16` holds the weights as the device keeps them, rounded
    to fp16 (nearest even) and widened again."""

    def __init__(self, weights, biases, input="binary"):
        if input not in _INPUTS:
            raise ValueError("input must be 'binary' or 'gray'")
        self.input = _INPUTS[input]
        self.weights = [np.ascontiguousarray(w, np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, np.float32).reshape(-1) for b in biases]
        if len(self.weights) != len(self.biases) or not self.weights:
            raise ValueError("a number model has 1 .. 3 layers, a weight and a bias each")
        if any(w.ndim != 2 for w in self.weights):
            raise ValueError("a layer's weight is [out][in]")
        self.dims = [int(self.weights[0].shape[1])] + [int(w.shape[0]) for w in self.weights]
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.shape != (self.dims[l + 1], self.dims[l]) or b.shape != (self.dims[l + 1],):
                raise ValueError(f"layer {l}: weight {w.shape} / bias {b.shape} do not chain to widths {self.dims}")
        check_shape(self.dims, self.input)
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            for what, a in (("weight", w), ("bias", b)):
                with np.errstate(invalid="ignore"):
                    if not (np.abs(a) <= np.float32(VALUE_MAX)).all():       # (a NaN fails)
                        raise ValueError(f"layer {l}: a {what} is not finite or above 65504 in magnitude")
        self.w16 = [w.astype(np.float16).astype(np.float32) for w in self.weights]

    @property
    def n_layers(self) -> int:
        return len(self.weights)

    @property
    def classes(self) -> int:
        return self.dims[-1]

    # ---- the kernel's arithmetic ----
    def inputs(self, gray: np.ndarray, otsu: np.ndarray):
        """(x float32 [n, 560], ones int64 [n])"""
        g = gray.astype(np.int64)
        if self.input == IN_GRAY:
            return gray.astype(np.float32) / np.float32(255.0), g.sum(1)
        one = g > otsu[:, None]
        return one.astype(np.float32), one.sum(1)

    @staticmethod
    def _layer(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
        """[n, in] -> [n, out]: four chains a unit, every operation a float32 one."""
        n, n_in = x.shape
        acc = np.zeros((n, w.shape[0], 4), np.float32)
        acc[:, :, 0] = b[None, :]
        for k0 in range(0, n_in, 4):
            m = min(4, n_in - k0)
            prod = w[None, :, k0:k0 + m] * x[:, None, k0:k0 + m]
            acc[:, :, :m] = acc[:, :, :m] + prod
        return (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])

    def logits(self, x: np.ndarray) -> np.ndarray:
        """x float32 [n, 560] -> logits float32 [n, C]"""
        a = np.ascontiguousarray(x, np.float32)
        for l in range(self.n_layers):
            if l:
                a = np.where(a > 0, a, np.float32(0.0)).astype(np.float32)
            a = self._layer(a, self.w16[l], self.biases[l])
        assert a.dtype == np.float32
        return a

    def reference(self, patches) -> np.ndarray:
        """The records (NUMBER_DTYPE [n], 96 bytes each) the kernel writes for these patch records."""
        gray, state, otsu = patch_arrays(patches)
        out = np.zeros(len(gray), NUMBER_DTYPE)
        live = np.flatnonzero(state == 1)
        if not len(live):
            return out
        x, ones = self.inputs(gray[live], otsu[live])
        lg = self.logits(x)
        C = self.classes
        rows = np.arange(len(live))
        label = np.argmax(lg, 1)                      # (the first of equal values)
        rec = np.zeros(len(live), NUMBER_DTYPE)
        rec["state"], rec["label"], rec["ones"] = 1, label, ones
        rec["logits"][:, :C] = lg
        if C > 1:
            rest = lg.copy()
            rest[rows, label] = -np.inf
            second = np.argmax(rest, 1)
            rec["second"] = second
            rec["margin"] = lg[rows, label] - lg[rows, second]
        else:
            rec["second"] = -1
        out[live] = rec
        return out

    def softmax(self, records) -> np.ndarray:
        """float32 [n, 16]: the softmax of each record's first C logits, in double; zero behind C and for "no answer"."""
        rec = np.asarray(records, NUMBER_DTYPE).reshape(-1)
        C = self.classes
        out = np.zeros((len(rec), CLASSES_MAX), np.float32)
        lg = rec["logits"][:, :C].astype(np.float64)
        e = np.exp(lg - lg.max(1, keepdims=True))
        out[:, :C] = (e / e.sum(1, keepdims=True)).astype(np.float32)
        out[rec["state"] != 1] = 0
        return out

    # ---- the .irmn file ----
    def to_bytes(self) -> bytes:
        dims = self.dims + [0] * (4 - len(self.dims))
        parts = [MAGIC, struct.pack("<Ii4ii", VERSION, self.n_layers, *dims, self.input)]
        for w, b in zip(self.weights, self.biases):
            parts += [w.astype("<f4").tobytes(), b.astype("<f4").tobytes()]
        return b"".join(parts)

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, data: bytes) -> "NumberModel":
        if len(data) < HEADER_BYTES or data[:4] != MAGIC:
            raise ValueError("not an .irmn file")
        version, n_layers, d0, d1, d2, d3, input_mode = struct.unpack("<Ii4ii", data[4:HEADER_BYTES])
        if version != VERSION:
            raise ValueError(f"unsupported .irmn version {version}")
        if not 1 <= n_layers <= LAYERS_MAX:
            raise ValueError("a number model has 1 .. 3 layers")
        dims = [d0, d1, d2, d3]
        if any(dims[n_layers + 1:]):
            raise ValueError("dims behind the last layer must be 0")
        dims = dims[:n_layers + 1]
        check_shape(dims, input_mode)          # (bounds every length below)
        need = sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(n_layers))
        if len(data) != HEADER_BYTES + 4 * need:
            raise ValueError(f"the file holds {len(data)} bytes, its header's model takes {HEADER_BYTES + 4 * need}")
        at, ws, bs = HEADER_BYTES, [], []
        for l in range(n_layers):
            nw = dims[l] * dims[l + 1]
            ws.append(np.frombuffer(data, "<f4", nw, at).reshape(dims[l + 1], dims[l])); at += 4 * nw
            bs.append(np.frombuffer(data, "<f4", dims[l + 1], at)); at += 4 * dims[l + 1]
        return cls(ws, bs, input_mode)

    @classmethod
    def load(cls, path: str) -> "NumberModel":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read())

    # ---- ONNX ----
    @classmethod
    def from_onnx(cls, onnx_bytes: bytes, input="binary", report: Optional[list] = None) -> "NumberModel":
        """A graph that is one chain of Flatten / Reshape, Gemm (transB 0 or 1, alpha = beta = 1) or MatMul + Add, Relu and
        an optional trailing Softmax (dropped, and noted in `report`).  Anything else is a ValueError that names the node."""
        from .onnx_import import _read_graph
        init, nodes = _read_graph(onnx_bytes)
        report = report if report is not None else []

        def who(n):
            return f"{n.name or (n.outputs[0] if n.outputs else '?')} ({n.op})"

        def tensor(n, name):
            if name not in init:
                raise ValueError(f"{who(n)}: input {name!r} is no initializer of the file")
            return np.asarray(init[name].array(), np.float64)

        ws: List[np.ndarray] = []
        bs: List[np.ndarray] = []
        relu_behind: List[bool] = []
        cur, pending = None, None          # the chain's value; a MatMul waiting for its Add
        for i, n in enumerate(nodes):
            data = [v for v in n.inputs if v not in init]
            if cur is not None and data[:1] != [cur]:
                raise ValueError(f"{who(n)}: the graph is no single chain (its input is not the output of the node in front)")
            if n.op in ("Flatten", "Reshape"):
                if ws:
                    raise ValueError(f"{who(n)}: only in front of the first layer")
            elif n.op == "Gemm":
                if (n.attrs.get("transA") or 0) != 0:
                    raise ValueError(f"{who(n)}: transA must be 0")
                for a in ("alpha", "beta"):
                    v = n.attrs.get(a)
                    if v is not None and float(v) != 1.0:
                        raise ValueError(f"{who(n)}: {a} must be 1")
                if len(n.inputs) < 2:
                    raise ValueError(f"{who(n)}: no weight")
                w = tensor(n, n.inputs[1])
                if w.ndim != 2:
                    raise ValueError(f"{who(n)}: the weight is not a matrix")
                w = w if (n.attrs.get("transB") or 0) == 1 else w.T
                ws.append(w)
                bs.append(tensor(n, n.inputs[2]).reshape(-1) if len(n.inputs) > 2 and n.inputs[2] else np.zeros(w.shape[0]))
                relu_behind.append(False)
            elif n.op == "MatMul":
                if len(n.inputs) != 2 or n.inputs[1] not in init:
                    raise ValueError(f"{who(n)}: the second input must be the weight, an initializer")
                w = tensor(n, n.inputs[1])
                if w.ndim != 2:
                    raise ValueError(f"{who(n)}: the weight is not a matrix")
                ws.append(w.T)
                bs.append(np.zeros(w.shape[1]))
                relu_behind.append(False)
                pending = len(ws) - 1
            elif n.op == "Add":
                if pending is None or pending != len(ws) - 1 or relu_behind[-1] or nodes[i - 1].op != "MatMul":
                    raise ValueError(f"{who(n)}: an Add is read only as the bias directly behind a MatMul")
                consts = [v for v in n.inputs if v in init]
                if len(consts) != 1:
                    raise ValueError(f"{who(n)}: one input must be the bias, an initializer")
                bs[-1] = tensor(n, consts[0]).reshape(-1)
                pending = None
            elif n.op == "Relu":
                if not ws or relu_behind[-1]:
                    raise ValueError(f"{who(n)}: a Relu is read only directly behind a layer")
                relu_behind[-1] = True
            elif n.op == "Softmax":
                if i != len(nodes) - 1 or not ws:
                    raise ValueError(f"{who(n)}: a Softmax is read only as the graph's last node")
                report.append(f"{who(n)}: dropped -- the records carry logits, softmax is the host's (NumberModel.softmax)")
            else:
                raise ValueError(f"{who(n)}: unsupported node; a number model is Flatten / Reshape, Gemm or MatMul + Add, Relu, Softmax")
            if not n.outputs:
                raise ValueError(f"{who(n)}: no output")
            cur = n.outputs[0]
        if not ws:
            raise ValueError("the graph has no Gemm or MatMul")
        if relu_behind[-1]:
            raise ValueError("the last layer carries a Relu: a number model's last layer gives the logits")
        if not all(relu_behind[:-1]):
            raise ValueError("a hidden layer carries no Relu: the kernel applies one behind every layer but the last")
        for l, (w, b) in enumerate(zip(ws, bs)):
            if b.shape != (w.shape[0],):
                raise ValueError(f"layer {l}: bias {b.shape} does not fit weight {w.shape}")
        report.append("layers " + " -> ".join(str(d) for d in [ws[0].shape[1]] + [w.shape[0] for w in ws]))
        with np.errstate(over="ignore"):
            return cls([w.astype(np.float32) for w in ws], [b.astype(np.float32) for b in bs], input)

    # ---- the C ABI ----
    def c_struct(self):
        """(capi.NumberModel, the arrays it points into): keep the second alive as long as the first is used."""
        import ctypes as C

        from . import capi
        m = capi.NumberModel()
        m.struct_size = C.sizeof(capi.NumberModel)
        m.n_layers, m.input = self.n_layers, self.input
        for l, d in enumerate(self.dims):
            m.dims[l] = d
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            m.weight[l] = w.ctypes.data_as(C.POINTER(C.c_float))
            m.bias[l] = b.ctypes.data_as(C.POINTER(C.c_float))
        return m, (self.weights, self.biases)


def records(numbers) -> np.ndarray:
    """capi.PlateNumber structures -> NUMBER_DTYPE [n]"""
    if not len(numbers):
        return np.zeros(0, NUMBER_DTYPE)
    return np.frombuffer(b"".join(bytes(r) for r in numbers), NUMBER_DTYPE).copy()


def main(argv) -> int:
    if len(argv) not in (3, 4) or (len(argv) == 4 and argv[3] not in ("binary", "gray")):
        print("usage: python -m irmv_detection_amd.number_net in.onnx out.irmn [binary|gray]", file=sys.stderr)
        return 2
    report: list = []
    with open(argv[1], "rb") as f:
        model = NumberModel.from_onnx(f.read(), argv[3] if len(argv) == 4 else "binary", report)
    model.save(argv[2])
    for line in report:
        print(line)
    print(f"wrote {argv[2]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
