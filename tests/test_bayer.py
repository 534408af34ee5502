"""Raw 8-bit Bayer input (include/irmv_hip.h IRMV_SRC_BAYER_*8): the host reference irmv_detection_amd/bayer.py, the C ABI
and facade surface (CPU), and on the GPU a Bayer engine against the same-config HWC engine fed bayer.demosaic(raw), bit for
bit, in every launch form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from irmv_detection_amd import _build, bayer, capi

PATTERNS = bayer.PATTERNS
SWAPPED = {"RGGB": "BGGR", "BGGR": "RGGB", "GRBG": "GBRG", "GBRG": "GRBG"}


# ---------------------------------------------------------------- host reference
def _demosaic_by_the_letter(raw, pattern):
    """Pixel-by-pixel transcription of the format's definition (include/irmv_hip.h), for the ramp tests."""
    H, W = raw.shape
    ry, rx = {"RGGB": (0, 0), "BGGR": (1, 1), "GRBG": (0, 1), "GBRG": (1, 0)}[pattern]

    def px(y, x):
        y = 1 if y < 0 else (H - 2 if y >= H else y)
        x = 1 if x < 0 else (W - 2 if x >= W else x)
        return int(raw[y, x])

    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            c = px(y, x)
            cross = (px(y - 1, x) + px(y + 1, x) + px(y, x - 1) + px(y, x + 1) + 2) >> 2
            diag = (px(y - 1, x - 1) + px(y - 1, x + 1) + px(y + 1, x - 1) + px(y + 1, x + 1) + 2) >> 2
            horiz = (px(y, x - 1) + px(y, x + 1) + 1) >> 1
            vert = (px(y - 1, x) + px(y + 1, x) + 1) >> 1
            r_row, r_col = (y & 1) == ry, (x & 1) == rx
            if r_row and r_col:
                out[y, x] = (c, cross, diag)
            elif not r_row and not r_col:
                out[y, x] = (diag, cross, c)
            elif r_row:
                out[y, x] = (horiz, c, vert)
            else:
                out[y, x] = (vert, c, horiz)
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
def test_constant_colour_round_trips_exactly(pattern):
    rgb = np.empty((6, 8, 3), np.uint8)
    rgb[:] = (200, 17, 90)
    assert np.array_equal(bayer.demosaic(bayer.mosaic(rgb, pattern), pattern), rgb)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("axis", [0, 1])
def test_ramps_match_the_formulas(pattern, axis):
    # odd steps: every two-neighbour sum is odd somewhere, so the half-up rounding is exercised
    n = np.arange(10)
    ramp = (7 + 23 * n) % 256 if axis == 1 else (250 - 27 * n) % 256
    raw = np.broadcast_to(ramp[None, :] if axis == 1 else ramp[:8, None], (8, 10)).astype(np.uint8).copy()
    got = bayer.demosaic(raw, pattern)
    assert np.array_equal(got, _demosaic_by_the_letter(raw, pattern))
    lin = np.broadcast_to((3 + 5 * n)[None, :], (8, 10)).astype(np.uint8)   # a linear ramp: the interior is reproduced exactly
    got = bayer.demosaic(np.ascontiguousarray(lin), pattern)
    assert np.array_equal(got[1:-1, 1:-1], np.repeat(lin[1:-1, 1:-1, None], 3, axis=2))


def test_hand_computed_4x4_reflect101_at_every_edge():
    raw = np.array([[10, 20, 30, 40],
                    [50, 60, 70, 80],
                    [90, 100, 110, 120],
                    [130, 140, 150, 160]], np.uint8)
    d = bayer.demosaic(raw, "RGGB")
    # (0,0) R site: N = S = row 1, W = E = column 1; every diagonal is (1,1)
    assert tuple(d[0, 0]) == (10, (50 + 50 + 20 + 20 + 2) >> 2, 60)
    # (0,3) G on the R row: E -> column 2, N -> row 1
    assert tuple(d[0, 3]) == (30, 40, 80)
    # (3,0) G on the B row: W -> column 1, S -> row 2
    assert tuple(d[3, 0]) == (90, 130, 140)
    # (3,3) B site: S -> row 2, E -> column 2, all four diagonals -> (2,2)
    assert tuple(d[3, 3]) == (110, (120 + 120 + 150 + 150 + 2) >> 2, 160)
    # interior B site and G site
    assert tuple(d[1, 1]) == (60, 60, 60)
    assert tuple(d[1, 2]) == (70, 70, 70)
    assert np.array_equal(d, _demosaic_by_the_letter(raw, "RGGB"))


def test_gains_identity_and_saturation():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, (16, 12), dtype=np.uint8)
    base = bayer.demosaic(raw, "GBRG")
    assert np.array_equal(bayer.demosaic(raw, "GBRG", (256, 256, 256)), base)
    g = bayer.demosaic(raw, "GBRG", (1023, 128, 300))
    b = base.astype(np.int64)
    assert np.array_equal(g[..., 0], np.minimum(255, (b[..., 0] * 1023 + 128) >> 8))
    assert np.array_equal(g[..., 1], (b[..., 1] * 128 + 128) >> 8)
    assert np.array_equal(g[..., 2], np.minimum(255, (b[..., 2] * 300 + 128) >> 8))
    full = np.full((4, 4), 255, np.uint8)
    assert (bayer.demosaic(full, "RGGB", (1023, 1023, 1023)) == 255).all()   # saturates at 255, never wraps
    with pytest.raises(ValueError):
        bayer.demosaic(raw, "GBRG", (1024, 256, 256))
    with pytest.raises(ValueError):
        bayer.demosaic(raw[:, :11], "GBRG")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_pattern_phase_on_rm_test_jpg(rm_test_image, pattern):
    def psnr(a, b):
        return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b) ** 2))
    raw = bayer.mosaic(rm_test_image, pattern)
    right = psnr(bayer.demosaic(raw, pattern), rm_test_image)
    wrong = psnr(bayer.demosaic(raw, SWAPPED[pattern]), rm_test_image)
    assert right >= 30.0 and wrong <= right - 10.0, (right, wrong)


# ---------------------------------------------------------------- C ABI (no GPU needed)
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def _cfg(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    return cfg


def test_cfg_default_is_hwc8_with_unit_gains(lib):
    cfg = _cfg(lib)
    assert cfg.struct_size == C.sizeof(capi.EngineCfg)
    assert cfg.src_format == capi.SRC_HWC8 and list(cfg.bayer_gain_q8) == [256, 256, 256]
    assert lib.irmv_engine_src_format(None) == -1 and lib.irmv_engine_src_bytes(None) == 0


def test_previous_struct_size_is_accepted_until_the_gpu_is_needed(lib):
    old = capi.EngineCfg.src_format.offset
    h = C.c_void_p()
    cfg = _cfg(lib)
    cfg.weights_path = b"/nonexistent/model.irmw"
    cfg.struct_size = old
    buf = C.create_string_buffer(bytes(C.string_at(C.addressof(cfg), old)), old)   # exactly the old struct's bytes
    rc = lib.irmv_engine_create(C.cast(buf, C.POINTER(capi.EngineCfg)), C.byref(h))
    assert rc in (capi.ERR_HIP, capi.ERR_MODEL), (rc, lib.irmv_last_error())
    assert b"size" not in lib.irmv_last_error()
    for bad in (old - 8, old + 8, C.sizeof(capi.EngineCfg) + 8, 4):
        cfg.struct_size = bad
        assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
        assert b"size mismatch" in lib.irmv_last_error()


@pytest.mark.parametrize("field,value,needle", [
    ("src_width", 1281, b"even"),
    ("src_height", 1023, b"even"),
    ("src_format", 5, b"src_format"),
    ("src_format", -1, b"src_format"),
    ("bayer_gain_q8", (256, 1024, 256), b"bayer_gain_q8"),
])
def test_bad_bayer_configs_are_rejected_before_touching_the_gpu(lib, field, value, needle):
    cfg = _cfg(lib)
    if field != "src_format":
        cfg.src_format = capi.SRC_BAYER_RGGB8
    if field == "bayer_gain_q8":
        cfg.bayer_gain_q8 = (C.c_uint16 * 3)(*value)
    else:
        setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
    assert needle in lib.irmv_last_error()
    if field in ("src_width", "bayer_gain_q8"):   # the same values are no error for an HWC8 engine
        cfg.src_format = capi.SRC_HWC8
        assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) != capi.ERR_ARG or b"Bayer" not in lib.irmv_last_error()


FACADE_SRC = r"""
#include <cstdio>
#include <cstring>
#include "irmv_detection/yolo_engine.hpp"

int main(int argc, char ** argv)
{
  if (argc < 3) return 2;
  // the camera SDK's CAMERA_MEDIA_TYPE_BAYGR8 buffer handed over as it is
  irmv_detection::YoloEngine engine(argv[1], cv::Size(1280, 1024), true, -1, false, -1, IRMV_SRC_BAYER_GRBG8, {300, 256, 420});
  FILE * f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  const size_t n = std::fread(engine.get_src_image_buffer(), 1, engine.src_image_bytes(), f);
  std::fclose(f);
  if (n != engine.src_image_bytes()) return 4;
  const auto bboxes = engine.detect();
  const cv::Mat & rotated = engine.get_rotated_image();
  std::printf("src_bytes %zu bboxes %zu rotated %d x %d type_ok %d\n", engine.src_image_bytes(), bboxes.size(), rotated.cols,
              rotated.rows, rotated.type() == CV_8UC3 ? 1 : 0);
  return 0;
}
"""


def _facade_exe():
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    os.makedirs(bindir, exist_ok=True)
    src = os.path.join(bindir, "bayer_facade_test.cpp")
    with open(src, "w") as f:
        f.write(FACADE_SRC)
    exe = os.path.join(bindir, "bayer_facade_test")
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_reference_style_bayer_code_compiles_against_the_facade():
    assert os.path.exists(_facade_exe())


# ---------------------------------------------------------------- GPU: Bayer engine == HWC engine on demosaic(raw)
def _frame(idx, w, h):
    from irmv_detection_amd import frames
    return frames.synthetic_frame(idx, w, h)


def _engine(blob, size, **kw):
    from irmv_detection_amd.engine import YoloEngine
    return YoloEngine(None, size, weights_blob=blob, **kw)


def _same_results(a, b):
    ra, rb = a.read_raw(a.slot), b.read_raw(b.slot)
    return ra["num_dets"] == rb["num_dets"] and all(np.array_equal(ra[k], rb[k]) for k in ("boxes", "scores", "classes", "anchors", "kpts"))


def _same_slot(a, sa, b, sb):
    ra, rb = a.read_raw(sa), b.read_raw(sb)
    if ra["num_dets"] != rb["num_dets"] or ra["n_candidates"] != rb["n_candidates"]:
        return False
    if not all(np.array_equal(ra[k], rb[k]) for k in ("boxes", "scores", "classes", "anchors", "kpts")):
        return False
    for x, y in zip(a.results(sa), b.results(sb)):
        if x.bbox_xyxy != y.bbox_xyxy or x.pnp_ok != y.pnp_ok or not np.array_equal(x.rvec, y.rvec) or not np.array_equal(x.tvec, y.tvec):
            return False
    return True


GEOMETRIES = [
    # (pattern, (W, H), net, resize_mode, rotate180, gains, backbone)
    ("RGGB", (1280, 1024), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),   # the reference configuration
    ("BGGR", (1280, 1024), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),
    ("GRBG", (1280, 1024), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),
    ("GBRG", (1280, 1024), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),
    ("GRBG", (640, 640), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),      # BASELINE configs[1]
    ("BGGR", (1280, 720), 640, capi.RESIZE_LETTERBOX, False, (256, 256, 256), "c2f"),
    ("GBRG", (642, 482), 640, capi.RESIZE_STRETCH, True, (256, 256, 256), "c2f"),      # W*H % 16 != 0: copy-engine upload, unaligned rows
    ("RGGB", (1280, 1024), 416, capi.RESIZE_STRETCH, True, (256, 256, 256), "shuffle"),   # ShuffleNetV2 backbone at 416
    ("RGGB", (1280, 1024), 640, capi.RESIZE_STRETCH, True, (600, 200, 1023), "c2f"),   # non-identity, saturating gains
]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,size,net,mode,rot,gains,backbone", GEOMETRIES)
def test_bayer_engine_is_bitwise_the_hwc_engine_on_the_demosaiced_frame(blob, pattern, size, net, mode, rot, gains, backbone):
    from irmv_detection_amd import arch, weights
    from oracle import oracle
    if backbone == "shuffle":
        blob = weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE)
    rgb = _frame(5, *size)
    raw = bayer.mosaic(rgb, pattern)
    hwc = bayer.demosaic(raw, pattern, gains)
    kw = dict(net_size=net, resize_mode=mode, rotate180=rot)
    with _engine(blob, size, src_format=pattern, bayer_gains=gains, **kw) as be, _engine(blob, size, **kw) as he:
        assert be.get_src_image_buffer().shape == (size[1], size[0])
        assert be._L.irmv_engine_src_bytes(be._h) == size[0] * size[1]
        assert be._L.irmv_engine_src_format(be._h) == capi.BAYER_FORMATS[pattern]
        be.get_src_image_buffer()[:] = raw
        he.get_src_image_buffer()[:] = hwc
        db, dh = be.detect(), he.detect()
        assert db == dh
        assert _same_slot(be, 0, he, 0)
        xb = be.read_input(0)
        assert np.array_equal(xb, he.read_input(0))
        assert np.array_equal(xb, oracle.preprocess(hwc, net, mode, rot).astype(np.float16).astype(np.float32))
        assert np.array_equal(be.read_head(0), he.read_head(0))
        assert np.array_equal(be.get_rotated_image(), hwc[::-1, ::-1])


@pytest.mark.gpu
def test_classical_extraction_on_mosaiced_rm_test_jpg(blob, rm_test_image):
    raw = bayer.mosaic(rm_test_image, "BGGR")
    hwc = bayer.demosaic(raw, "BGGR")
    rng = np.random.default_rng(5)
    xy0 = rng.uniform(0, 1100, (24, 2))
    boxes = np.concatenate([xy0, xy0 + rng.uniform(40, 300, (24, 2))], axis=1).astype(np.float32)
    boxes = np.concatenate([boxes, np.array([[0, 0, 1280, 1024], [300, 200, 900, 800]], np.float32)])
    with _engine(blob, (1280, 1024), src_format=capi.SRC_BAYER_BGGR8) as be, _engine(blob, (1280, 1024)) as he:
        be.get_src_image_buffer()[:] = raw
        he.get_src_image_buffer()[:] = hwc
        ab, ah = be.extract_armors(boxes), he.extract_armors(boxes)
        assert len(ab) == len(ah) == len(boxes)
        for x, y in zip(ab, ah):
            assert (x.valid, x.n_lights, x.size, x.pnp_ok, x.no_answer) == (y.valid, y.n_lights, y.size, y.pnp_ok, y.no_answer)
            assert np.array_equal(x.image_points(), y.image_points())
            assert np.array_equal(x.rvec, y.rvec) and np.array_equal(x.tvec, y.tvec)
        assert sum(a.valid for a in ah) > 0


def _hip_memcpy_h2d(dst_ptr, arr):
    """hipMemcpy through the HIP runtime libirmv_hip.so already loaded (same SONAME: dlopen returns that library)."""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(arr)
    assert hip.hipMemcpy(C.c_void_p(dst_ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice


@pytest.mark.gpu
def test_every_launch_form_gives_the_same_bits(blob, monkeypatch):
    pattern = "GRBG"
    raws = [bayer.mosaic(_frame(40 + i, 1280, 1024), pattern) for i in range(8)]
    # reference: an HWC engine on the demosaiced frames, one synchronous detect() per slot
    with _engine(blob, (1280, 1024), num_slots=8, num_streams=2) as he:
        for s in range(8):
            he.get_src_image_buffer(s)[:] = bayer.demosaic(raws[s], pattern)
            he.detect(s)
        forms = {}
        for mode in ("graph", "eager"):
            monkeypatch.setenv("IRMV_SYNC_LAUNCH", mode)
            with _engine(blob, (1280, 1024), src_format=pattern, num_slots=8, num_streams=2) as be:
                assert be.sync_launch == mode
                for s in range(8):
                    be.get_src_image_buffer(s)[:] = raws[s]
                    be.detect(s)
                    assert _same_slot(be, s, he, s), (mode, s)
                forms[mode] = True
                if mode == "eager":
                    continue
                # batched submit(H2D): 8 slots on 2 streams
                for s in range(8):
                    be.get_src_image_buffer((s + 3) % 8)[:] = raws[s]
                be.submit(0, 8)
                be.wait()
                for s in range(8):
                    assert _same_slot(be, (s + 3) % 8, he, s), ("batched", s)
                # ASYNC_UPLOAD pipelining: slot n + 1 uploads while slot n runs
                for s in range(8):
                    be.get_src_image_buffer(s)[:] = raws[7 - s]
                for s in range(8):
                    be.submit(s, 1, async_upload=True)
                for s in range(8):
                    be.wait_slots(s, 1)
                    assert _same_slot(be, s, he, 7 - s), ("async", s)
                be.wait()
                # a device-resident producer: raw frames written into the device slots, submitted without H2D
                for s in range(8):
                    be.get_src_image_buffer(s)[:] = 0
                    _hip_memcpy_h2d(be.src_device_ptr(s), raws[s])
                be.submit(0, 8, h2d=False)
                be.wait()
                for s in range(8):
                    assert _same_slot(be, s, he, s), ("device", s)
                be.submit(2, 1, h2d=False)
                be.wait()
                assert _same_slot(be, 2, he, 2)
    monkeypatch.delenv("IRMV_SYNC_LAUNCH")
    assert set(forms) == {"graph", "eager"}


@pytest.mark.gpu
def test_profile_lists_the_demosaic_only_for_bayer_engines(blob, monkeypatch):
    # An engine times its candidates at creation (conv tiles; one grouped launch for a Detect branch against separate ones) and
    # keeps the faster: two engines may differ where two candidates time alike.  What is compared here is the step's SHAPE, so
    # both engines take the untimed choices.
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_FORCE", "1")
    with _engine(blob, (1280, 1024)) as he:
        hwc_names = [k["name"] for k in he.profile(0, 1)]
    assert hwc_names and not any("demosaic" in n for n in hwc_names)
    with _engine(blob, (1280, 1024), src_format=capi.SRC_BAYER_RGGB8) as be:
        prof = be.profile(0, 1)
    assert [k["name"] for k in prof] == ["bayer_demosaic"] + hwc_names   # one op in front of the unchanged step
    assert prof[0]["bytes"] == 1280 * 1024 * 4 and prof[0]["ms"] > 0


@pytest.mark.gpu
def test_facade_runs_a_bayer_engine(tmp_path, blob):
    exe = _facade_exe()
    (tmp_path / "m.irmw").write_bytes(blob)
    bayer.mosaic(_frame(2, 1280, 1024), "GRBG").tofile(tmp_path / "raw.bin")
    out = subprocess.run([exe, str(tmp_path / "m.onnx"), str(tmp_path / "raw.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "src_bytes 1310720" in out.stdout and "rotated 1280 x 1024 type_ok 1" in out.stdout
