"""Rectangular network input (irmv_engine_cfg.net_height), the parts that need no GPU: the C ABI's struct versions and
validation, and the host references tests/test_gpu_rect.py checks the engine against (tests/rect_ref.py), each proven
against the square oracle where both apply."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rect_ref
from conftest import ROOT
from irmv_detection_amd import _build, capi, frames
from oracle import oracle


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def _cfg(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    cfg.weights_path = b"/nonexistent/model.irmw"
    return cfg


def _create(lib, cfg, size=None, raw=None):
    """irmv_engine_create on exactly `size` bytes of cfg (raw: those bytes as given)."""
    size = C.sizeof(cfg) if size is None else size
    data = raw if raw is not None else bytes(C.string_at(C.addressof(cfg), min(size, C.sizeof(cfg)))).ljust(size, b"\0")
    buf = C.create_string_buffer(data, max(size, C.sizeof(capi.EngineCfg)))
    h = C.c_void_p()
    rc = lib.irmv_engine_create(C.cast(buf, C.POINTER(capi.EngineCfg)), C.byref(h))
    if rc == capi.OK:
        lib.irmv_engine_destroy(h)
    return rc, lib.irmv_last_error()


def test_cfg_default_is_square_and_sizes_agree_with_the_header(lib, tmp_path):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    assert cfg.net_height == 0 and cfg.net_size == 640 and cfg.struct_size == C.sizeof(capi.EngineCfg) == 280
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(irmv_engine_cfg), offsetof(irmv_engine_cfg, net_height), offsetof(irmv_engine_cfg, reserved2));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.EngineCfg), capi.EngineCfg.net_height.offset, capi.EngineCfg.reserved2.offset] == [280, 268, 272]


@pytest.mark.parametrize("size", [256, 272, 280])
def test_every_struct_version_is_accepted_until_the_gpu_is_needed(lib, size):
    cfg = _cfg(lib)
    cfg.struct_size = size
    rc, msg = _create(lib, cfg, size)
    assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (rc, msg)
    assert b"size" not in msg


@pytest.mark.parametrize("size", [264, 276, 288])
def test_other_struct_sizes_are_refused(lib, size):
    cfg = _cfg(lib)
    cfg.struct_size = size
    rc, msg = _create(lib, cfg, size)
    assert rc == capi.ERR_ARG and b"size mismatch" in msg


def test_previous_header_tail_bytes_are_not_read(lib):
    """A 272-byte struct (the header before net_height): whatever bytes 268..271 hold, the engine is square -- here,
    validation passes where an out-of-range net_height would be refused."""
    cfg = _cfg(lib)
    cfg.struct_size = 272
    raw = bytearray(C.string_at(C.addressof(cfg), 272))
    raw[268:272] = b"\xff\x7f\x13\x99"
    rc, msg = _create(lib, cfg, 272, bytes(raw))
    assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (rc, msg)
    assert b"net_height" not in msg
    cfg.struct_size = 280
    cfg.net_height = int.from_bytes(raw[268:272], "little", signed=True)   # the same bytes in the new header ARE read
    rc, msg = _create(lib, cfg)
    assert rc == capi.ERR_ARG and b"net_height" in msg


@pytest.mark.parametrize("h", [48, 100, 4096, -32, 32, 2080])
def test_bad_net_height_is_refused_naming_the_field(lib, h):
    cfg = _cfg(lib)
    cfg.net_height = h
    rc, msg = _create(lib, cfg)
    assert rc == capi.ERR_ARG and b"net_height" in msg, (rc, msg)


@pytest.mark.parametrize("h", [0, 64, 512, 2048])
def test_good_net_height_passes_validation(lib, h):
    cfg = _cfg(lib)
    cfg.net_height = h
    rc, msg = _create(lib, cfg)
    assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (rc, msg)


def test_net_dims_refuses_a_null_engine(lib):
    w, h = C.c_int(-1), C.c_int(-1)
    assert lib.irmv_engine_net_dims(None, C.byref(w), C.byref(h)) == capi.ERR_ARG


# ---- the preprocess restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,net,mode,rot,swap", [
    ((1280, 1024), 640, 0, True, False), ((1280, 1024), 640, 0, False, True), ((1280, 1024), 640, 1, True, False),
    ((1280, 1024), 416, 1, False, True), ((641, 479), 320, 0, True, False), ((333, 1000), 256, 1, False, False),
    ((1276, 1280), 640, 1, True, True), ((640, 640), 640, 0, True, False),
])
def test_preprocess_restatement_is_the_oracle_at_square_sizes(size, net, mode, rot, swap):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    img[: size[1] // 2] = frames.synthetic_frame(2, size[0], size[1])[: size[1] // 2]
    out, u8 = oracle.preprocess(img, net, mode, rot, swap, want_u8=True)
    assert np.array_equal(rect_ref.preprocess_u8(img, net, net, mode, rot, swap), u8)
    assert np.array_equal(rect_ref.preprocess(img, net, net, mode, rot, swap), out.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("W,H,expect", [
    (640, 512, (640, 512, 0, 0)),        # 5 : 4 camera, 5 : 4 input: no padding
    (640, 480, (600, 480, 20, 0)),
    (416, 352, (416, 333, 0, 9)),
    (320, 640, (320, 256, 0, 192)),
    (640, 640, (640, 512, 0, 64)),       # the square letterbox: 64 grey rows above and below
])
def test_letterbox_geometry_for_the_1280x1024_camera(W, H, expect):
    assert rect_ref.letterbox_geom(1280, 1024, W, H) == expect


def test_rect_preprocess_of_a_2_to_1_input_is_pair_averages():
    """640 x 512 from 1280 x 1024 (stretch, no rotation): every output pixel is the rounded mean of a 2 x 2 source block."""
    img = frames.synthetic_frame(1)
    q = rect_ref.preprocess_u8(img, 640, 512, 0, False, False).astype(np.int64)
    blk = img.astype(np.int64).reshape(512, 2, 640, 2, 3).sum((1, 3))
    assert np.array_equal(q, (blk * 512 + (1 << 10)) >> 11)
    assert rect_ref.preprocess_u8(img, 640, 512, 1, False, False).tobytes() == q.astype(np.uint8).tobytes()


# ---- the embedded-square decode / NMS ------------------------------------------------------------------------------------
def _head(rng, A, hot=0.004, nc=14, nk=8):
    head = np.zeros((A, 64 + nc + nk), np.float32)
    head[:, :64] = rng.standard_normal((A, 64)) - 0.4 * (np.arange(64) % 16)
    cls = rng.standard_normal((A, nc)) - 6.0
    m = rng.random((A, nc)) < hot
    cls[m] = rng.uniform(-1.0, 4.0, m.sum())
    head[:, 64:64 + nc] = cls
    head[:, 64 + nc:] = 0.25 + 0.3 * rng.standard_normal((A, nk))
    return head


@pytest.mark.parametrize("net", [640, 416, 96])
def test_embedding_is_the_identity_for_square_heads(net):
    assert np.array_equal(rect_ref.anchor_map(net, net), np.arange(rect_ref.num_anchors(net, net)))
    head = _head(np.random.default_rng(net), rect_ref.num_anchors(net, net))
    a, b = rect_ref.decode_nms(head, net, net, 14, 8), oracle.decode_nms(head, net, 14, 8)
    assert a["num_dets"] == b["num_dets"] > 0 and a["n_candidates"] == b["n_candidates"]
    for k in ("anchors", "boxes", "scores", "classes", "kpts"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("W,H", [(640, 512), (416, 352), (320, 640), (224, 96)])
def test_embedded_decode_matches_a_direct_decode(W, H):
    A = rect_ref.num_anchors(W, H)
    assert A == {(640, 512): 6720, (416, 352): 3003}.get((W, H), A)
    rng = np.random.default_rng(W * 7 + H)
    head = _head(rng, A, hot=0.01)
    amap = rect_ref.anchor_map(W, H)
    assert (np.diff(amap) > 0).all()
    S = max(W, H)
    boxes_sq, keys = oracle.decode_candidates(rect_ref.embed_square(head, W, H, 14), S, 14, 8)
    direct = rect_ref.decode_boxes(head, W, H)
    assert np.abs(boxes_sq[amap] - direct).max() < 1e-3                    # every rect anchor's box, decoded in its square slot
    cls = head[:, 64:78]
    assert len(keys) == int((cls > float(np.log(0.25 / 0.75))).sum())        # exactly the rect candidates, none from the filler
    d = rect_ref.decode_nms(head, W, H, 14, 8)
    assert d["num_dets"] > 0
    assert np.abs(d["boxes"] - direct[d["anchors"]]).max() < 1e-3
    cx, cy, st = rect_ref.anchor_grid(W, H)
    kp = head[d["anchors"], 78:86]
    want = np.stack([(2 * kp[:, 0::2] + (cx[d["anchors"], None] - 0.5)) * st[d["anchors"], None],
                     (2 * kp[:, 1::2] + (cy[d["anchors"], None] - 0.5)) * st[d["anchors"], None]], 2).reshape(-1, 8)
    assert np.abs(d["kpts"] - want).max() < 1e-3
    assert (np.diff(d["scores"]) <= 0).all()


def test_parse_output_restatement_is_the_oracle_at_square_sizes():
    b = np.random.default_rng(1).uniform(-20, 660, (50, 4)).astype(np.float32)
    for mode in (0, 1):
        assert np.array_equal(rect_ref.parse_output(b, 1280, 1024, 640, 640, mode), oracle.parse_output(b, 1280, 1024, 640, mode))
