"""The ONNX importer on files it did not write: serialized by google.protobuf (tests/onnx_files.py) in every encoding an
export can use, with and without the graph, and the files it must refuse."""
import re

import numpy as np
import pytest

import checkpoint
import onnx_files
from irmv_detection_amd import arch, onnx_import, weights

MODELS = {"pose": dict(), "bbox": dict(nk=0), "shuffle": dict(backbone=arch.BACKBONE_SHUFFLE)}


@pytest.fixture(scope="module")
def models():
    out = {}
    for tag, kw in MODELS.items():
        specs, tensors = weights.synthetic_tensors(0, **kw)
        out[tag] = (specs, onnx_files.named(specs, tensors), kw.get("nk", 8), kw.get("backbone", arch.BACKBONE_C2F))
    return out


def _expected(model, encoding):
    specs, named, nk, backbone = model
    return weights.build_blob(specs, checkpoint.expected_tensors(named, onnx_files.stored_dtype(encoding), specs), 14, nk, backbone)


# ---- blob equality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(MODELS))
@pytest.mark.parametrize("encoding", list(onnx_files.ENCODINGS))
def test_every_encoding_imports_to_the_expected_blob(models, encoding, tag):
    """Byte for byte, in file order and shuffled, with and without what an export carries besides, with and without nodes."""
    want = _expected(models[tag], encoding)
    named = models[tag][1]
    for order, extras, nodes in ((None, True, "ultralytics"), (5, False, None), (7, True, None), (11, False, "ultralytics")):
        data = onnx_files.write_model(named, encoding, nodes=nodes, extras=extras, order=order)
        assert onnx_import.convert(data) == want, (order, extras, nodes)


def test_the_fp32_encodings_reproduce_the_synthetic_blob(models, blob):
    """(the expected blob is not a restatement of the importer: for fp32 files it is the blob the weights came from)"""
    for enc in ("raw32", "float_data", "dims_packed", "raw64", "double_data"):
        assert _expected(models["pose"], enc) == blob


def test_fp16_files_round_the_biases_once_through_fp16(models):
    specs, named, _, _ = models["pose"]
    _, layers = weights.parse_blob(onnx_import.convert(onnx_files.write_model(named, "int32_fp16")))
    n_moved = 0
    for (sp, w, b), (w0, b0) in zip(layers, weights.synthetic_tensors(0)[1]):
        assert np.array_equal(w, w0)
        assert np.array_equal(b, b0.astype(np.float16).astype(np.float32))
        n_moved += int((b != b0).sum())
    assert n_moved > 1000


def test_unpacked_repeated_fields_are_read_too(models):
    """proto2 readers must accept both forms of a repeated scalar: one key per element instead of one packed field."""
    specs, named, _, _ = models["pose"]
    enc = onnx_import._enc_varint
    name = "model.22.cv4.0.2.bias"
    b = named[name].astype(np.float32)
    by_hand = {}
    t32 = b"".join(enc((1 << 3) | 0) + enc(d) for d in b.shape) + enc((2 << 3) | 0) + enc(1) + onnx_import._enc_field(8, name.encode())
    by_hand["float"] = t32 + b"".join(enc((4 << 3) | 5) + v.tobytes() for v in b)
    t16 = b"".join(enc((1 << 3) | 0) + enc(d) for d in b.shape) + enc((2 << 3) | 0) + enc(10) + onnx_import._enc_field(8, name.encode())
    by_hand["half"] = t16 + b"".join(enc((5 << 3) | 0) + enc(int(v)) for v in b.astype(np.float16).view(np.uint16))
    for kind, payload in by_hand.items():
        t = onnx_files.PB["TensorProto"].FromString(payload)       # the real parser reads the hand-made bytes the same way
        assert len(t.float_data if kind == "float" else t.int32_data) == 8
        graph = b"".join(onnx_import._enc_field(5, payload if n == name else onnx_files.tensor_proto(onnx_files.PB, n, a).SerializeToString())
                         for n, a in named.items())
        out = onnx_import.convert(enc((1 << 3) | 0) + enc(8) + onnx_import._enc_field(7, graph))
        got = dict((sp.name, bb) for sp, _, bb in weights.parse_blob(out)[1])["model.22.cv4.0.2"]
        assert np.array_equal(got, b if kind == "float" else b.astype(np.float16).astype(np.float32))


# ---- rounding -------------------------------------------------------------------------------------------------------
EDGE = np.array([1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30), 1 + 3 * 2.0 ** -11 - 2.0 ** -30,
                 2.0 ** -14 * (1 + 2.0 ** -11 + 2.0 ** -40), 2.0 ** -24 * (1.5 - 2.0 ** -30), 2.0 ** -25 * (1 + 2.0 ** -30)])


@pytest.mark.parametrize("encoding", ["raw64", "double_data"])
def test_fp64_weights_are_rounded_to_fp16_once(models, encoding):
    """fp64 values within 2^-24 relative of an fp16 rounding tie: fp32 cannot tell them from the tie, so the detour
    fp64 -> fp32 -> fp16 rounds them to even where the direct rounding goes to the nearer neighbour."""
    direct, detour = EDGE.astype(np.float16), EDGE.astype(np.float32).astype(np.float16)
    assert (direct != detour).all()
    assert float(direct[0]) == 1 + 2.0 ** -10 and float(detour[0]) == 1.0
    specs, named, _, _ = models["pose"]
    named = dict(named)
    w = named["model.0.conv.weight"].astype(np.float64)
    w[3, 1, 0, :3], w[15, 2, 2, :3] = EDGE[:3], EDGE[3:]
    named["model.0.conv.weight"] = w
    out = onnx_import.convert(onnx_files.write_model(named, encoding, nodes="ultralytics"))
    w16 = weights.parse_blob(out)[1][0][1]                                          # OHWI
    assert np.array_equal(w16[3, 0, :3, 1], direct[:3]) and np.array_equal(w16[15, 2, :3, 2], direct[3:])
    assert out == weights.build_blob(specs, checkpoint.expected_tensors(named, np.float64, specs), 14, 8)


@pytest.mark.parametrize("encoding", ["raw32", "raw64"])
def test_the_largest_weight_that_stays_finite(models, encoding):
    """65519.9 is below the midpoint 65520 of the largest fp16 and the first value that is out of range: it imports as 65504."""
    named = dict(models["pose"][1])
    w = named["model.4.cv1.conv.weight"].astype(np.float64)
    w[17, 5, 0, 0], w[18, 5, 0, 0] = 65519.9, -65519.9
    named["model.4.cv1.conv.weight"] = w
    rep = []
    out = onnx_import.convert(onnx_files.write_model(named, encoding), rep)
    w16 = dict((sp.name, ww) for sp, ww, _ in weights.parse_blob(out)[1])["model.4.cv1"]
    assert float(w16[17, 0, 0, 5]) == 65504.0 and float(w16[18, 0, 0, 5]) == -65504.0
    assert dict((r[0], r[3]) for r in rep)["model.4.cv1"] == pytest.approx(65519.9, rel=1e-6)


# ---- refusals -------------------------------------------------------------------------------------------------------
def _with_value(named, name, index, value, dtype=np.float32):
    named = dict(named)
    a = named[name].astype(dtype).copy()
    a[index] = value
    named[name] = a
    return named


def _refusals(named):
    """tag -> (file, what the message must say)"""
    pb = onnx_files.PB
    wname = "model.6.m.1.cv2.conv.weight"                   # [64, 64, 3, 3]
    ext = onnx_files.tensor_proto(pb, wname, named[wname])
    ext.ClearField("raw_data")
    ext.data_location = 1
    ext.external_data.add(key="location", value="model.onnx.data")
    ext_entry_only = onnx_files.tensor_proto(pb, wname, named[wname])
    ext_entry_only.ClearField("raw_data")
    ext_entry_only.external_data.add(key="location", value="model.onnx.data")
    bf16 = onnx_files.tensor_proto(pb, wname, named[wname], "raw16", onnx_type=onnx_files.BFLOAT16)
    permuted = onnx_files.tensor_proto(pb, wname, named[wname].transpose(0, 2, 3, 1))
    short = onnx_files.tensor_proto(pb, wname, named[wname])
    short.raw_data = short.raw_data[:-4]
    bn = dict(named)
    for k, v in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0)):
        bn["model.0.bn." + k] = np.full(16, v, np.float32)
    W = lambda **kw: onnx_files.write_model(kw.pop("named", named), kw.pop("encoding", "raw32"), **kw)
    return {
        "external data": (W(replace={wname: ext}), r"model\.6\.m\.1\.cv2\.conv\.weight.*external"),
        "external_data entry alone": (W(replace={wname: ext_entry_only}), r"model\.6\.m\.1\.cv2\.conv\.weight.*external"),
        "bfloat16": (W(replace={wname: bf16}), r"model\.6\.m\.1\.cv2\.conv\.weight.*data_type 16 \(BFLOAT16\)"),
        "1e5": (W(named=_with_value(named, wname, (37, 2, 1, 1), 1e5)), r"model\.6\.m\.1\.cv2: output channel 37 .*fp16 infinity"),
        "65520": (W(named=_with_value(named, wname, (63, 0, 0, 0), -65520.0)), r"model\.6\.m\.1\.cv2: output channel 63 .*fp16 infinity"),
        "NaN": (W(named=_with_value(named, wname, (16, 63, 2, 2), np.nan)), r"model\.6\.m\.1\.cv2: output channel 16 .*NaN or Inf"),
        "Inf in an fp16 file": (W(named=_with_value(named, wname, (0, 0, 0, 0), np.inf), encoding="int32_fp16"),
                                r"model\.6\.m\.1\.cv2: output channel 0 .*NaN or Inf"),
        "NaN bias": (W(named=_with_value(named, "model.22.cv3.1.2.bias", 13, np.nan)), r"model\.22\.cv3\.1\.2: the bias of output channel 13"),
        "fp64 bias beyond fp32": (W(named=_with_value(named, "model.9.cv2.conv.bias", 255, 1e39, np.float64), encoding="raw64"),
                                  r"model\.9\.cv2: the bias of output channel 255"),
        "permuted dims": (W(replace={wname: permuted}), r"model\.6\.m\.1\.cv2: shape \(64, 3, 3, 64\) does not match"),
        "short payload": (W(replace={wname: short}), r"model\.6\.m\.1\.cv2\.conv\.weight: raw_data holds 147452 bytes"),
        "missing bias": (W(replace={"model.6.m.1.cv2.conv.bias": None}), r"model\.6\.m\.1\.cv2.*has no model\.6\.m\.1\.cv2\.conv\.bias"),
        "leftover BN": (W(named=bn), r"model\.0\.bn\..*export with fused BatchNorm"),
        "stride 1 where 2 is due": (W(nodes="ultralytics", overrides={"model.3.conv": dict(strides=[1, 1])}),
                                    r"model\.3\.conv: Conv strides = \[1, 1\].*\[2, 2\]"),
        "asymmetric pads": (W(nodes="ultralytics", overrides={"model.22.cv2.1.0": dict(pads=[1, 1, 0, 0])}), r"model\.22\.cv2\.1\.0: Conv pads"),
        "grouped conv": (W(nodes="ultralytics", overrides={"model.8.cv1": dict(group=2)}), r"model\.8\.cv1: Conv group = 2"),
        "ReLU export": (W(nodes="ultralytics", activation="relu"), r"model\.0\.conv: .*Relu.*not by SiLU"),
    }


def test_each_bad_file_is_refused_in_its_own_words(models):
    named = models["pose"][1]
    cases = _refusals(named)
    said = {}
    for tag, (data, pattern) in cases.items():
        with pytest.raises(ValueError, match=pattern) as ei:           # (a refusal: no blob comes back)
            onnx_import.convert(data)
        said[tag] = str(ei.value)
    groups = [{"1e5", "65520"}, {"external data", "external_data entry alone"}, {"NaN", "Inf in an fp16 file"},
              {"NaN bias", "fp64 bias beyond fp32"}]               # the same fault in two files: the same words
    for tag, (_, pattern) in cases.items():
        for other, msg in said.items():
            if other != tag and not any(tag in g and other in g for g in groups):
                assert not re.search(pattern, msg), (tag, other, msg)
    assert len(set(said.values())) >= len(said) - len(groups)
    assert "not found" not in " ".join(said.values()) and "YOLOv8" not in " ".join(said.values())


def test_a_sigmoid_behind_a_final_and_a_batchnorm_node_are_refused(models):
    named = models["pose"][1]
    data = onnx_files.write_model(named, "raw32", nodes="ultralytics")
    m = onnx_files.PB["ModelProto"].FromString(data)
    final = next(n for n in m.graph.node if n.op_type == "Conv" and n.input[1] == "model.22.cv3.0.2.weight")
    m.graph.node.add(op_type="Sigmoid", input=[final.output[0]], output=["/scores"], name="/model.22/Sigmoid")
    with pytest.raises(ValueError, match=r"model\.22\.cv3\.0\.2: the Conv feeds a Sigmoid"):
        onnx_import.convert(m.SerializeToString())
    m = onnx_files.PB["ModelProto"].FromString(data)
    m.graph.node.add(op_type="BatchNormalization", input=["x"], output=["y"], name="/model.0/bn/BatchNormalization")
    with pytest.raises(ValueError, match="export with fused BatchNorm"):
        onnx_import.convert(m.SerializeToString())


# ---- truncation -------------------------------------------------------------------------------------------------------
def test_a_file_cut_short_is_refused_wherever_the_cut_falls(models):
    """64 cuts over a raw32 file: inside the first bytes, inside tensors, three bytes before the end of the last tensor, and
    in what follows the graph.  (A cut that falls exactly between two top-level fields after the graph leaves a complete
    ModelProto with the whole graph -- a valid file; such positions are moved one byte on.)"""
    data = onnx_files.write_model(models["pose"][1], "raw32", nodes="ultralytics")
    assert onnx_import.convert(data)
    m = onnx_files.PB["ModelProto"].FromString(data)
    g = m.graph.SerializeToString()
    graph_end = data.index(g[:64]) + len(g)
    assert data[graph_end - len(g):graph_end] == g and graph_end < len(data) - 40    # opset_import and metadata_props follow
    last = m.graph.initializer[-1].raw_data
    last_end = data.rindex(last) + len(last)
    boundaries, p = set(), graph_end
    for entry in list(m.opset_import) + list(m.metadata_props):
        boundaries.add(p)
        p += 2 + len(entry.SerializeToString())
    assert p == len(data)
    cuts = set(int(v) for v in np.linspace(1, len(data) - 1, 56))
    cuts |= {2, 3, last_end - len(last) + 5, last_end - 3, last_end, graph_end - 1, graph_end + 1, graph_end + 3, len(data) - 3, len(data) - 1}
    cuts = sorted(c + 1 if c in boundaries else c for c in cuts)
    assert len(cuts) >= 64 and sum(c > graph_end for c in cuts) >= 4
    for c in cuts:
        with pytest.raises(ValueError):
            onnx_import.convert(data[:c])


def test_a_nested_field_that_overruns_its_parent_is_refused(models):
    """Not a cut of the file: the parents' lengths are right, a tensor inside claims more bytes than its own message has."""
    name, f = "model.22.cv4.0.2.bias", onnx_import._enc_field
    whole = onnx_files.tensor_proto(onnx_files.PB, name, models["pose"][1][name]).SerializeToString()
    for tensor in (whole[:-3], whole[:len(whole) - 32 - 1]):
        data = onnx_import._enc_varint((1 << 3) | 0) + onnx_import._enc_varint(8) + f(7, f(5, tensor))
        with pytest.raises(ValueError, match="truncated protobuf"):
            onnx_import.convert(data)
    node = f(1, f(1, b"x") + f(5, f(1, b"strides") + onnx_import._enc_varint((8 << 3) | 2) + b"\x05\x02"))     # ints: 5 bytes announced, 1 there
    with pytest.raises(ValueError, match="truncated protobuf"):
        onnx_import.convert(onnx_import._enc_varint((1 << 3) | 0) + onnx_import._enc_varint(8) + f(7, node))


# ---- report -----------------------------------------------------------------------------------------------------------
def test_report_is_empty_handed_on_the_synthetic_blob(models, tmp_path, capsys):
    rep = []
    onnx_import.convert(onnx_files.write_model(models["pose"][1], "raw32"), rep)
    assert [r[0] for r in rep] == [sp.name for sp in models["pose"][0]]
    assert all(r[1] == 0 and r[2] == 0 and 0 < r[3] < 16 for r in rep)
    p = tmp_path / "m.onnx"
    p.write_bytes(onnx_files.write_model(models["pose"][1], "raw32"))
    assert onnx_import.main(["prog", str(p)]) == 0
    assert "subnormal" not in capsys.readouterr().out


def test_the_package_imports_without_protobuf():
    import subprocess
    import sys
    code = ("import sys; sys.modules['google'] = None; sys.modules['google.protobuf'] = None\n"
            "from irmv_detection_amd import onnx_import\n"
            "assert not any(k.startswith('google') and v is not None for k, v in sys.modules.items())\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=onnx_files.__file__.rsplit("/tests/", 1)[0])
