"""Plate numbers on the host (include/irmv_hip.h, "plate numbers"): irmv_detection_amd.number_net -- the reference the GPU
tests demand bytes of -- against an independent restatement, the derived forward bound of the single-layer model, the edge
cases of the model, the .irmn file through both readers (Python's and the library's, which needs no GPU), the ONNX import on
real protobuf files, and the three structs against their ctypes mirrors.

The restatement is written in another shape than `NumberModel.reference`: one patch at a time, one input k at a time in a
plain loop, every product and every sum computed in float64 and cast to float32 -- the correctly rounded float32 operation,
since 53 >= 2 * 24 + 2 -- and the chains kept as four separate accumulators.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import onnx_files as OF
from conftest import ROOT
from irmv_detection_amd import _build, capi, number_net as NN, patches as PT

N_PATCHES = 200
SHAPES = ([560, 9], [560, 64, 9], [560, 128, 100, 16])


def make_model(dims, seed=0, input="binary", scale=None):
    r = np.random.RandomState(100 + seed)
    ws, bs = [], []
    for l in range(len(dims) - 1):
        s = scale if scale is not None else 1.0 / np.sqrt(max(dims[l], 1))
        ws.append((r.standard_normal((dims[l + 1], dims[l])) * s).astype(np.float32))
        bs.append((r.standard_normal(dims[l + 1]) * 0.5).astype(np.float32))
    return NN.NumberModel(ws, bs, input)


def seeded_patches(n=N_PATCHES, seed=7):
    """(gray [n, 560] uint8, state [n], otsu [n]): smooth structure plus noise at several contrasts, each with its own Otsu
    threshold (patches.otsu); every tenth has state 0, and a few are one-level."""
    r = np.random.RandomState(seed)
    j, i = np.mgrid[0:28, 0:20].astype(np.float64)
    gray = np.empty((n, 560), np.uint8)
    otsu = np.empty(n, np.int64)
    for p in range(n):
        a, c = r.uniform(5, 120), r.uniform(20, 235)
        img = c + a * np.sin(r.uniform(0.1, 0.9) * i + r.uniform(0.1, 0.9) * j + r.uniform(0, 6.28)) + r.uniform(-a / 3, a / 3, i.shape)
        if p % 37 == 5:
            img[:] = r.randint(0, 256)
        gray[p] = np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(-1)
        otsu[p] = PT.otsu(gray[p])[0]
    state = (np.arange(n) % 10 != 3).astype(np.int64)
    return gray, state, otsu


@pytest.fixture(scope="module")
def patches():
    return seeded_patches()


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def restated_logits(model, gray, otsu):
    """One patch: the logits as float32, by float64 operations cast to float32 one at a time."""
    if model.input == NN.IN_BINARY:
        x = [1.0 if int(g) > int(otsu) else 0.0 for g in gray]
    else:
        x = [float(f32(float(g) / 255.0)) for g in gray]            # (two float32 values: the float64 quotient cast is the float32 one)
    a = np.array(x, np.float64)
    for l in range(model.n_layers):
        if l:
            a = np.array([v if v > 0 else 0.0 for v in a], np.float64)
        wt = model.weights[l].astype(np.float16).astype(np.float64).T      # [in][out]
        chain = [model.biases[l].astype(np.float64)] + [np.zeros(model.dims[l + 1]) for _ in range(3)]
        for k in range(model.dims[l]):
            chain[k % 4] = f32(chain[k % 4] + f32(wt[k] * a[k]))
        a = f32(f32(chain[0] + chain[1]) + f32(chain[2] + chain[3]))
    return a.astype(np.float32)


def restated_record(model, gray, state, otsu):
    rec = np.zeros((), NN.NUMBER_DTYPE)
    if state != 1:
        return rec
    lg = restated_logits(model, gray, otsu)
    C_ = model.classes
    order = sorted(range(C_), key=lambda c: (-float(lg[c]), c))
    rec["state"], rec["label"] = 1, order[0]
    rec["second"] = order[1] if C_ > 1 else -1
    rec["margin"] = np.float32(np.float64(lg[order[0]]) - np.float64(lg[order[1]])) if C_ > 1 else np.float32(0)
    rec["ones"] = sum(int(g) > int(otsu) for g in gray) if model.input == NN.IN_BINARY else sum(int(g) for g in gray)
    rec["logits"][:C_] = lg
    return rec


# ---- 1. the reference against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("input", ["binary", "gray"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_reference_equals_the_scalar_restatement_in_bytes(patches, dims, input):
    gray, state, otsu = patches
    model = make_model(dims, len(dims), input)
    ref = model.reference(patches)
    assert ref.dtype == NN.NUMBER_DTYPE and len(ref) == N_PATCHES >= 200
    for p in range(N_PATCHES):
        want = restated_record(model, gray[p], state[p], otsu[p])
        assert ref[p].tobytes() == want.tobytes(), (p, ref[p], want)
    assert (ref["state"] == state).all() and (ref[state == 0].view(np.uint8) == 0).all()
    assert len({r.tobytes() for r in ref["logits"][state == 1]}) >= 150          # (not one answer for everything)


@pytest.mark.parametrize("input", ["binary", "gray"])
def test_single_layer_forward_error_bound(patches, input):
    """|fp32 logit - float64 logit| <= 561 * 2^-24 * (|b| + sum |w_k x_k|): the forward bound of a 561-term sum of rounded
    products, whatever the order of the additions."""
    gray, state, otsu = patches
    model = make_model([560, 9], 2, input)
    ref = model.reference(patches)
    x, _ = model.inputs(gray, otsu)
    w, b = model.w16[0].astype(np.float64), model.biases[0].astype(np.float64)
    exact = x.astype(np.float64) @ w.T + b
    bound = 561 * 2.0 ** -24 * (np.abs(b)[None, :] + np.abs(x.astype(np.float64))[:, None, :].__mul__(np.abs(w)[None]).sum(2))
    live = state == 1
    err = np.abs(ref["logits"][:, :9].astype(np.float64) - exact)
    assert (err[live] <= bound[live]).all(), float((err[live] / bound[live]).max())
    assert err[live].max() > 0          # (the float32 arithmetic is visible at all)


# ---- 2. edge cases ------------------------------------------------------------------------------------------------------------
def one_patch(gray_value=None, otsu=100, seed=3):
    r = np.random.RandomState(seed)
    g = r.randint(0, 256, (1, 560)).astype(np.uint8) if gray_value is None else np.full((1, 560), gray_value, np.uint8)
    return g, np.array([1]), np.array([otsu])


def test_ties_go_to_the_smaller_index():
    r = np.random.RandomState(5)
    w = (r.standard_normal((6, 560)) * 0.05).astype(np.float32)
    b = np.zeros(6, np.float32)
    w[4] = w[1]                                   # two identical rows ...
    w[[0, 2, 3, 5]] -= 1.0                        # ... above every other one on any input with a one in it
    rec = NN.NumberModel([w], [b]).reference(one_patch())[0]
    assert rec["logits"][1] == rec["logits"][4] and (rec["label"], rec["second"], rec["margin"]) == (1, 4, 0.0)
    w3 = np.tile(w[1], (3, 1))                    # all equal: 0, then 1
    rec = NN.NumberModel([w3], [np.zeros(3, np.float32)]).reference(one_patch())[0]
    assert (rec["label"], rec["second"], rec["margin"]) == (0, 1, 0.0)


def test_one_class():
    m = make_model([560, 7, 1], 1)
    rec = m.reference(one_patch())[0]
    assert (rec["state"], rec["label"], rec["second"], rec["margin"]) == (1, 0, -1, 0.0)
    assert rec["logits"][0] == restated_logits(m, *[a[0] for a in (one_patch()[0], one_patch()[2])])[0] and not rec["logits"][1:].any()
    assert m.softmax(m.reference(one_patch()))[0, 0] == 1.0


def test_relu_of_minus_zero_is_plus_zero():
    """ReLU is a > 0 ? a : +0: -0 and every negative value feed +0 on.  (A unit's sum itself is never -0: three of its four
    chains start at +0 and +0 + -0 = +0; the case below drives a hidden unit as close as the model allows -- bias -0, weights
    -0, every input 1 -- and a second one to -3.)"""
    x = np.array([[-0.0, -3.0, 0.0, 2.5, -1e-45]], np.float32)
    h = np.where(x > 0, x, np.float32(0.0)).astype(np.float32)          # (what logits() applies between the layers)
    assert h.tobytes() == np.array([[0.0, 0.0, 0.0, 2.5, 0.0]], np.float32).tobytes()
    w1, b1 = np.full((2, 560), -0.0, np.float32), np.array([-0.0, -3.0], np.float32)
    w2, b2 = np.array([[-1.0, 0.0], [0.0, -1.0]], np.float32), np.array([-0.0, -0.0], np.float32)
    m = NN.NumberModel([w1, w2], [b1, b2])
    one = one_patch(gray_value=255, otsu=0)
    x1, ones = m.inputs(one[0], one[2])
    assert ones[0] == 560
    hidden = m._layer(x1, m.w16[0], m.biases[0])
    assert hidden.tobytes() == np.array([[0.0, -3.0]], np.float32).tobytes()
    rec = m.reference(one)[0]
    assert rec["logits"][:2].tobytes() == restated_logits(m, one[0][0], 0).tobytes() == np.zeros(2, np.float32).tobytes()


def test_fp16_subnormal_weights_are_kept():
    tiny = np.float32(2.0 ** -24)                 # the smallest fp16 subnormal
    w = np.full((2, 560), tiny, np.float32)
    w[1] = np.float32(2.0 ** -25) * np.float32(1.5)   # rounds to 2^-24 (nearest), 2^-25 itself to zero (even)
    m = NN.NumberModel([w], [np.zeros(2, np.float32)])
    assert (m.w16[0] == tiny).all()
    assert (NN.NumberModel([np.full((1, 560), 2.0 ** -25, np.float32)], [np.zeros(1, np.float32)]).w16[0] == 0).all()
    rec = m.reference(one_patch(gray_value=255, otsu=3))[0]
    assert rec["ones"] == 560 and rec["logits"][0] == np.float32(560 * 2.0 ** -24) and rec["logits"][1] == rec["logits"][0]
    g = NN.NumberModel([w], [np.zeros(2, np.float32)], "gray").reference(one_patch(gray_value=1, otsu=0))[0]
    assert g["ones"] == 560 and g["logits"][0] > 0          # products of 2^-24 / 255: nothing flushed


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def c_set_model(lib, model_like):
    """irmv_engine_set_number_model(NULL engine, model): the values are checked first, so a refused value answers before the
    engine is looked at and a good model gets as far as 'engine is null'."""
    m, keep = model_like.c_struct()
    rc = lib.irmv_engine_set_number_model(None, C.byref(m))
    return rc, lib.irmv_last_error().decode()


class Raw:
    """A model the Python checks have not seen."""
    def __init__(self, weights, biases, input=0):
        self.weights = [np.ascontiguousarray(w, np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, np.float32) for b in biases]
        self.dims = [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]
        self.n_layers, self.input = len(self.weights), input
    c_struct = NN.NumberModel.c_struct


def test_value_bound_and_non_finite_values_are_refused(lib):
    w, b = np.zeros((3, 560), np.float32), np.zeros(3, np.float32)
    ok = Raw([w], [b])
    rc, msg = c_set_model(lib, ok)
    assert rc == capi.ERR_ARG and "engine is null" in msg
    edge = w.copy(); edge[1, 7] = 65504.0; edge[2, 9] = -65504.0
    assert "engine is null" in c_set_model(lib, Raw([edge], [np.array([65504, -65504, 0], np.float32)]))[1]
    assert NN.NumberModel([edge], [b]).w16[0][1, 7] == 65504.0
    for bad in (np.nextafter(np.float32(65504), np.float32(np.inf)), -65520.0, np.inf, -np.inf, np.nan):
        for where in ("weight", "bias"):
            w2, b2 = w.copy(), b.copy()
            if where == "weight":
                w2[2, 559] = bad
            else:
                b2[2] = bad
            with pytest.raises(ValueError, match=where):
                NN.NumberModel([w2], [b2])
            rc, msg = c_set_model(lib, Raw([w2], [b2]))
            assert rc == capi.ERR_ARG and where in msg, (bad, where, msg)
    # shapes
    for dims in ([559, 3], [560, 17], [560, 129, 3], [560, 0, 3], [560, 4, 4, 4, 4]):
        with pytest.raises(ValueError):
            make_model(dims)
    rc, msg = c_set_model(lib, Raw([np.zeros((17, 560), np.float32)], [np.zeros(17, np.float32)]))
    assert rc == capi.ERR_ARG and "1 .. 16" in msg
    rc, msg = c_set_model(lib, Raw([np.zeros((129, 560), np.float32), np.zeros((2, 129), np.float32)], [np.zeros(129, np.float32), np.zeros(2, np.float32)]))
    assert rc == capi.ERR_ARG and "1 .. 128" in msg
    rc, msg = c_set_model(lib, Raw([w], [b], input=2))
    assert rc == capi.ERR_ARG and "input" in msg
    lim = (C.c_int32 * 8)()
    assert lib.irmv_number_limits(lim) == 0
    assert list(lim) == [560, 128, 16, 3, 96, 560 * 128 + 128 * 128 + 128 * 16, 65504, 0]
    assert (NN.N_IN, NN.HIDDEN_MAX, NN.CLASSES_MAX, NN.LAYERS_MAX) == tuple(lim[:4])


# ---- 3. the .irmn file ------------------------------------------------------------------------------------------------------
def c_read(lib, path):
    m = capi.NumberModel()
    need = C.c_int64(-1)
    buf = np.zeros(90384, np.float32)
    rc = lib.irmv_number_model_read(os.fsencode(path), C.byref(m), buf.ctypes.data_as(C.POINTER(C.c_float)), len(buf), C.byref(need))
    return rc, m, buf, need.value


@pytest.mark.parametrize("dims", SHAPES + ([560, 1], [560, 128, 128, 16]), ids=lambda d: "-".join(map(str, d)))
def test_irmn_round_trip_in_bytes(lib, tmp_path, dims):
    model = make_model(dims, 9, "gray" if len(dims) == 3 else "binary")
    path = str(tmp_path / "m.irmn")
    model.save(path)
    data = open(path, "rb").read()
    assert len(data) == 32 + 4 * sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1))
    back = NN.NumberModel.load(path)
    assert back.to_bytes() == data and back.dims == model.dims and back.input == model.input
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back.weights + back.biases, model.weights + model.biases))
    rc, m, buf, need = c_read(lib, path)
    assert rc == 0 and need == (len(data) - 32) // 4 <= 90384
    assert (m.struct_size, m.n_layers, m.input) == (C.sizeof(capi.NumberModel), model.n_layers, model.input)
    assert list(m.dims) == dims + [0] * (4 - len(dims))
    assert buf[:need].tobytes() == data[32:]
    for l in range(model.n_layers):
        assert np.ctypeslib.as_array(m.weight[l], (dims[l + 1] * dims[l],)).tobytes() == model.weights[l].tobytes()
        assert np.ctypeslib.as_array(m.bias[l], (dims[l + 1],)).tobytes() == model.biases[l].tobytes()


def test_irmn_files_that_are_refused(lib, tmp_path):
    data = make_model([560, 64, 9]).to_bytes()

    def both(blob, name):
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        with pytest.raises(ValueError):
            NN.NumberModel.from_bytes(blob)
        rc = c_read(lib, p)[0]
        assert rc in (capi.ERR_ARG, capi.ERR_MODEL), name
        assert lib.irmv_engine_load_number_model(None, os.fsencode(p)) == rc      # (refused before the engine is looked at)

    both(data[:-1], "cut1")                                   # truncated
    both(data[:32 + 4 * 560 * 10], "cut_in_layer0")
    both(data[:20], "cut_in_header")
    both(b"", "empty")
    both(data + b"\0\0\0\0", "longer")
    both(b"IRMX" + data[4:], "magic")
    both(data[:4] + (2).to_bytes(4, "little") + data[8:], "version")
    # oversized dims: each would index far past the file if a length were used before it is checked
    for at, v in ((8, 4), (8, 1 << 30), (12, 561), (16, 129), (16, 1 << 30), (20, 17), (20, -5), (24, 1), (28, 2)):
        both(data[:at] + int(v).to_bytes(4, "little", signed=True) + data[at + 4:], f"field{at}_{v}")
    assert c_read(lib, str(tmp_path / "nothing_here"))[0] == capi.ERR_MODEL
    rc, m, buf, need = c_read(lib, str(tmp_path / "cut1"))
    small = np.zeros(16, np.float32)                          # a buffer that is too small: refused, and told how much it takes
    p = str(tmp_path / "good"); open(p, "wb").write(data)
    need = C.c_int64(0)
    assert lib.irmv_number_model_read(os.fsencode(p), C.byref(capi.NumberModel()), small.ctypes.data_as(C.POINTER(C.c_float)), 16, C.byref(need)) == capi.ERR_ARG
    assert need.value == (len(data) - 32) // 4 and not small.any()


def test_softmax_helper_and_the_library_agree(lib, patches):
    model = make_model([560, 64, 9], 4)
    ref = model.reference(patches)
    sm = model.softmax(ref)
    assert sm.shape == (N_PATCHES, 16) and not sm[:, 9:].any() and not sm[ref["state"] == 0].any()
    assert np.allclose(sm[ref["state"] == 1].sum(1), 1.0, atol=1e-6) and (np.argmax(sm[ref["state"] == 1], 1) == ref["label"][ref["state"] == 1]).all()
    out = (C.c_float * 16)()
    for p in (0, 1, 2, 3, 50):
        rec = capi.PlateNumber.from_buffer_copy(ref[p].tobytes())
        assert lib.irmv_number_softmax(C.byref(rec), 9, out) == 0
        assert np.array_equal(np.array(list(out), np.float32), sm[p])
    big = np.zeros(1, NN.NUMBER_DTYPE); big["state"] = 1; big["logits"][0, :2] = (3.0e21, -3.0e21)      # no overflow in double
    assert list(make_model([560, 2]).softmax(big)[0, :2]) == [1.0, 0.0]
    assert lib.irmv_number_softmax(None, 9, out) == capi.ERR_ARG and lib.irmv_number_softmax(C.byref(rec), 17, out) == capi.ERR_ARG


# ---- 4. from_onnx on real protobuf files ----------------------------------------------------------------------------------------
def onnx_mlp(model, form, softmax=False, flatten="Flatten", pb=OF.PB, extra=None):
    """The model as an ONNX file out of google.protobuf: form 'gemm1' (transB = 1, weight [out][in]), 'gemm0' (no transB,
    weight [in][out]) or 'matmul' (MatMul + Add)."""
    nodes, inits, cur = [], [], "input"

    def node(op, inputs, **attrs):
        nonlocal cur
        out = f"/{op}_{len(nodes)}_output_0"
        nd = pb["NodeProto"](name=f"/{op}_{len(nodes)}", op_type=op, input=inputs, output=[out])
        nd.attribute.extend(OF._attr(pb, k, v) for k, v in attrs.items())
        nodes.append(nd)
        cur = out

    if flatten == "Flatten":
        node("Flatten", [cur], axis=1)
    elif flatten == "Reshape":
        inits.append(OF.tensor_proto(pb, "shape", np.array([-1, 560], np.int64)))
        node("Reshape", [cur, "shape"])
    for l, (w, b) in enumerate(zip(model.weights, model.biases)):
        if extra and extra[0] == l:
            node(extra[1], [cur])
        if form == "gemm1":
            inits += [OF.tensor_proto(pb, f"fc{l}.weight", w), OF.tensor_proto(pb, f"fc{l}.bias", b)]
            node("Gemm", [cur, f"fc{l}.weight", f"fc{l}.bias"], alpha=1.0, beta=1.0, transB=1)
        elif form == "gemm0":
            inits += [OF.tensor_proto(pb, f"fc{l}.weight", np.ascontiguousarray(w.T)), OF.tensor_proto(pb, f"fc{l}.bias", b)]
            node("Gemm", [cur, f"fc{l}.weight", f"fc{l}.bias"])
        else:
            inits += [OF.tensor_proto(pb, f"fc{l}.w", np.ascontiguousarray(w.T)), OF.tensor_proto(pb, f"fc{l}.b", b)]
            node("MatMul", [cur, f"fc{l}.w"])
            node("Add", [f"fc{l}.b", cur] if l & 1 else [cur, f"fc{l}.b"])
        if l < model.n_layers - 1:
            node("Relu", [cur])
    if softmax:
        node("Softmax", [cur], axis=1)
    g = pb["GraphProto"](name="mlp", node=nodes, initializer=inits, input=[pb["ValueInfoProto"](name="input")],
                         output=[pb["ValueInfoProto"](name=cur)])
    return pb["ModelProto"](ir_version=8, producer_name="test", graph=g, opset_import=[pb["OperatorSetIdProto"](domain="", version=13)]).SerializeToString()


@pytest.mark.parametrize("softmax", [False, True], ids=["logits", "softmax"])
@pytest.mark.parametrize("form", ["gemm1", "gemm0", "matmul"])
def test_from_onnx_gives_the_direct_models_logits(patches, form, softmax):
    for dims, flatten, pb in (([560, 9], "Flatten", OF.PB), ([560, 64, 9], "Reshape", OF.PB_DIMS_PACKED), ([560, 128, 100, 16], None, OF.PB)):
        direct = make_model(dims, 11, "gray")
        report = []
        got = NN.NumberModel.from_onnx(onnx_mlp(direct, form, softmax, flatten, pb), "gray", report)
        assert got.dims == direct.dims and got.to_bytes() == direct.to_bytes()
        sub = tuple(a[:40] for a in patches)
        assert got.reference(sub).tobytes() == direct.reference(sub).tobytes()
        assert any("Softmax" in line and "dropped" in line for line in report) == softmax


def test_from_onnx_refuses_what_it_does_not_read(tmp_path):
    m = make_model([560, 64, 9], 12)
    with pytest.raises(ValueError, match=r"/Conv_1 \(Conv\)"):
        NN.NumberModel.from_onnx(onnx_mlp(m, "gemm1", extra=(0, "Conv")))
    with pytest.raises(ValueError, match="Sigmoid"):
        NN.NumberModel.from_onnx(onnx_mlp(m, "matmul", extra=(1, "Sigmoid")))
    pb = OF.PB
    m1 = make_model([560, 9], 13)
    w, b = OF.tensor_proto(pb, "w", m1.weights[0]), OF.tensor_proto(pb, "b", m1.biases[0])

    def graph(*nodes):
        return pb["ModelProto"](graph=pb["GraphProto"](node=list(nodes), initializer=[w, b])).SerializeToString()

    def gemm(**attrs):
        nd = pb["NodeProto"](name="/fc", op_type="Gemm", input=["x", "w", "b"], output=["y"])
        nd.attribute.extend(OF._attr(pb, k, v) for k, v in attrs.items())
        return nd

    assert NN.NumberModel.from_onnx(graph(gemm(transB=1))).to_bytes() == m1.to_bytes()
    for attrs, what in ((dict(transB=1, alpha=0.5), "alpha"), (dict(transB=1, beta=2.0), "beta"), (dict(transB=1, transA=1), "transA")):
        with pytest.raises(ValueError, match=what):
            NN.NumberModel.from_onnx(graph(gemm(**attrs)))
    relu = pb["NodeProto"](name="/act", op_type="Relu", input=["y"], output=["z"])
    with pytest.raises(ValueError, match="last layer"):
        NN.NumberModel.from_onnx(graph(gemm(transB=1), relu))
    with pytest.raises(ValueError, match="hidden layer carries no Relu"):      # two layers without a Relu between them
        NN.NumberModel.from_onnx(_no_relu(m))
    # the command line
    src, dst = tmp_path / "m.onnx", tmp_path / "m.irmn"
    src.write_bytes(onnx_mlp(m, "gemm1", softmax=True))
    out = subprocess.check_output([os.sys.executable, "-m", "irmv_detection_amd.number_net", str(src), str(dst)], cwd=ROOT, text=True)
    assert "dropped" in out and dst.read_bytes() == m.to_bytes()


def _no_relu(m):
    pb = OF.PB
    inits = [OF.tensor_proto(pb, "w0", m.weights[0]), OF.tensor_proto(pb, "b0", m.biases[0]), OF.tensor_proto(pb, "w1", m.weights[1]), OF.tensor_proto(pb, "b1", m.biases[1])]
    n0 = pb["NodeProto"](name="/fc0", op_type="Gemm", input=["x", "w0", "b0"], output=["h"])
    n1 = pb["NodeProto"](name="/fc1", op_type="Gemm", input=["h", "w1", "b1"], output=["y"])
    for n in (n0, n1):
        n.attribute.extend([OF._attr(pb, "transB", 1)])
    return pb["ModelProto"](graph=pb["GraphProto"](node=[n0, n1], initializer=inits)).SerializeToString()


# ---- 5. the structs against their mirrors ----------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    pairs = (("irmv_plate_number", capi.PlateNumber), ("irmv_number_model", capi.NumberModel), ("irmv_number_opts", capi.NumberOpts))
    parts = []
    for cname, mirror in pairs:
        parts.append(f'printf(" %zu", sizeof({cname}));')
        parts += [f'printf(" %zu %zu", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));' for f, _ in mirror._fields_]
    src = tmp_path / "nm.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(parts) +
                   'printf(" %d %d %d", IRMV_NUM_IN_BINARY, IRMV_NUM_IN_GRAY, IRMV_NUM_CLASSES_MAX);return 0;}\n')
    exe = tmp_path / "nm"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, mirror in pairs:
        want.append(C.sizeof(mirror))
        for f, _ in mirror._fields_:
            want += [getattr(mirror, f).offset, getattr(mirror, f).size]
    want += [capi.NUM_IN_BINARY, capi.NUM_IN_GRAY, capi.NUM_CLASSES_MAX]
    assert got == want
    assert C.sizeof(capi.PlateNumber) == 96 == NN.NUMBER_DTYPE.itemsize
    assert [NN.NUMBER_DTYPE.fields[f][1] for f in NN.NUMBER_DTYPE.names] == [getattr(capi.PlateNumber, f).offset for f, _ in capi.PlateNumber._fields_]
    assert (NN.IN_BINARY, NN.IN_GRAY) == (capi.NUM_IN_BINARY, capi.NUM_IN_GRAY)
