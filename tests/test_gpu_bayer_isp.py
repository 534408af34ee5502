"""The Bayer ISP on the GPU: the Malvar-He-Cutler kernel against bayer.demosaic(algo="mhc") bit for bit, an MHC engine's
whole step against the HWC engine on the host-demosaiced frame, and irmv_engine_set_bayer_isp on a living engine in every
launch form (synchronous graph / eager, batched, per-share, asynchronous upload, rotated_image, extract_armors)."""
import ctypes
import subprocess

import numpy as np
import pytest

import bayer_isp_ref as ref
from irmv_detection_amd import bayer, capi

pytestmark = pytest.mark.gpu

SIZE = (1280, 1024)
LUT = ref.gamma_lut(0.5)
GAINS = ref.GAINS
UNIT = (256, 256, 256)


def _frame(idx, w=SIZE[0], h=SIZE[1]):
    from irmv_detection_amd import frames
    return frames.synthetic_frame(idx, w, h)


def _engine(blob, size=SIZE, **kw):
    from irmv_detection_amd.engine import YoloEngine
    return YoloEngine(None, size, weights_blob=blob, **kw)


def _snap(e, slot=0):
    """Everything a step left for one slot, as arrays of its own."""
    r = e.read_raw(slot)
    d = {k: np.array(r[k]) for k in ("boxes", "scores", "classes", "anchors", "kpts")}
    d["counts"] = np.array([r["num_dets"], r["n_candidates"]])
    d["pose"] = np.array([np.concatenate([a.rvec, a.tvec, [a.pnp_ok]]) for a in e.results(slot)]).reshape(-1, 7)
    d["head"] = e.read_head(slot)
    return d


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------- frame parity of the MHC kernel
# (W, H) of the source.  The net is 64 x 64, the smallest there is: irmv_front_plan takes every one of these sizes at it
# (6 x 4 and 18 x 10 with the three unfused front kernels, widths that are no multiple of 4).
SMALL = [(4, 4), (6, 4), (18, 10)]
FRAME_CASES = ([(s, p, UNIT, None) for s in SMALL for p in bayer.PATTERNS] +
               [((20, 18), "BGGR", UNIT, None), ((32, 16), "GRBG", UNIT, None), ((48, 8), "GBRG", UNIT, None),
                ((320, 256), "RGGB", UNIT, None), ((320, 256), "GRBG", (600, 200, 1023), "gamma")])


@pytest.mark.parametrize("size,pattern,gains,lut", FRAME_CASES, ids=[f"{s[0]}x{s[1]}-{p}-{'isp' if l else 'unit'}" for s, p, _, l in FRAME_CASES])
def test_mhc_frame_is_the_host_reference(blob, monkeypatch, size, pattern, gains, lut):
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")        # the frame does not depend on the conv tiles: skip their timing
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    raw = rng.integers(0, 256, (size[1], size[0]), dtype=np.uint8)
    table = None if lut is None else np.stack([LUT, 255 - LUT, np.roll(LUT, 7)])
    with _engine(blob, size, net_size=64, src_format=pattern, bayer_gains=gains, bayer_demosaic="mhc") as e:
        assert e.bayer_demosaic == "mhc"
        if table is not None:
            e.set_bayer_isp(gains, table)
        e.get_src_image_buffer()[:] = raw
        got = e.get_rotated_image()[::-1, ::-1]
        assert np.array_equal(got, bayer.demosaic(raw, pattern, gains, "mhc", table))
        g, t = e.bayer_isp
        assert g == tuple(gains) and np.array_equal(t, table if table is not None else np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256)))


def test_bilinear_table_kernel_frame_is_the_host_reference(blob, monkeypatch):
    """The table form of the bilinear kernel (an engine after its first set) at the sizes where its paths part: with an
    identity LUT it gives the bits of the argument-gain kernel, with a LUT those of the host reference."""
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    for size, pattern in (((2, 2), "RGGB"), ((18, 10), "GBRG"), ((32, 16), "BGGR"), ((320, 256), "GRBG")):
        raw = np.random.default_rng(size[0]).integers(0, 256, (size[1], size[0]), dtype=np.uint8)
        with _engine(blob, size, net_size=64, src_format=pattern, bayer_gains=(600, 200, 1023)) as e:
            e.get_src_image_buffer()[:] = raw
            before = e.get_rotated_image()
            assert np.array_equal(before[::-1, ::-1], bayer.demosaic(raw, pattern, (600, 200, 1023)))
            e.set_bayer_isp((600, 200, 1023))
            assert np.array_equal(e.get_rotated_image(), before)
            e.set_bayer_isp(GAINS, LUT)
            assert np.array_equal(e.get_rotated_image()[::-1, ::-1], bayer.demosaic(raw, pattern, GAINS, lut=LUT))


# ---------------------------------------------------------------- results parity: MHC engine == HWC engine on demosaic(raw)
def _geometries():
    from test_bayer import GEOMETRIES
    g = [GEOMETRIES[0], GEOMETRIES[5]]             # stretch + rotate at 1280 x 1024, and the letterbox geometry (1280 x 720)
    assert g[0][3] == capi.RESIZE_STRETCH and g[0][4] and g[1][3] == capi.RESIZE_LETTERBOX
    return [(p, size, net, None, mode, rot) for p, size, net, mode, rot, _, _ in g] + [("GBRG", (1280, 1024), 640, 512, capi.RESIZE_LETTERBOX, True)]


@pytest.mark.parametrize("pattern,size,net,net_h,mode,rot", _geometries())
def test_mhc_engine_is_bitwise_the_hwc_engine_on_the_demosaiced_frame(blob, pattern, size, net, net_h, mode, rot):
    raw = bayer.mosaic(_frame(5, *size), pattern)
    hwc = bayer.demosaic(raw, pattern, GAINS, "mhc", LUT)
    kw = dict(net_size=net, net_height=net_h, resize_mode=mode, rotate180=rot)
    with _engine(blob, size, src_format=pattern, bayer_demosaic="mhc", **kw) as be, _engine(blob, size, **kw) as he:
        be.set_bayer_isp(GAINS, LUT)
        be.get_src_image_buffer()[:] = raw
        he.get_src_image_buffer()[:] = hwc
        assert be.detect() == he.detect()
        assert np.array_equal(be.read_input(0), he.read_input(0))
        assert _same(_snap(be), _snap(he))
        assert np.array_equal(be.get_rotated_image(), hwc[::-1, ::-1])


def test_mhc_batched_submit_is_bitwise_the_hwc_engine(blob):
    pattern = "BGGR"
    raws = [bayer.mosaic(_frame(60 + i), pattern) for i in range(4)]
    with _engine(blob, src_format=pattern, bayer_demosaic="mhc", num_slots=4) as be, _engine(blob, num_slots=4) as he:
        for s in range(4):
            be.get_src_image_buffer(s)[:] = raws[s]
            he.get_src_image_buffer(s)[:] = bayer.demosaic(raws[s], pattern, algo="mhc")
        be.submit(0, 4)
        he.submit(0, 4)
        be.wait()
        he.wait()
        for s in range(4):
            assert _same(_snap(be, s), _snap(he, s)), s


# ---------------------------------------------------------------- live update
PATTERN = "GRBG"


@pytest.fixture(scope="module")
def live():
    """Eight raw frames and their host-demosaiced frames without and with the ISP.  Each test below feeds them to an HWC
    engine of its own engine's shape (slots, streams, submit form), so the two sides run the same kernels."""
    raws = [bayer.mosaic(_frame(40 + i), PATTERN) for i in range(8)]
    return dict(raws=raws, base=[bayer.demosaic(r, PATTERN) for r in raws], isp=[bayer.demosaic(r, PATTERN, GAINS, lut=LUT) for r in raws])


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_live_update_reaches_a_synchronous_detect(blob, live, monkeypatch, mode):
    monkeypatch.setenv("IRMV_SYNC_LAUNCH", mode)
    with _engine(blob, src_format=PATTERN) as be, _engine(blob) as he:
        assert be.sync_launch == mode
        he.get_src_image_buffer()[:] = live["base"][0]
        he.detect()
        want_base = _snap(he)
        he.get_src_image_buffer()[:] = live["isp"][0]
        he.detect()
        want_isp = _snap(he)
        assert not _same(want_base, want_isp)                    # the ISP changes what the network sees
        be.get_src_image_buffer()[:] = live["raws"][0]
        be.detect()
        first = _snap(be)
        assert _same(first, want_base)
        be.set_bayer_isp(GAINS, LUT)
        assert be.bayer_isp[0] == GAINS and np.array_equal(be.bayer_isp[1], np.broadcast_to(LUT, (3, 256)))
        be.detect()
        assert _same(_snap(be), want_isp)
        be.detect()
        assert _same(_snap(be), want_isp)
        be.set_bayer_isp(UNIT)
        be.detect()
        assert _same(_snap(be), first)


@pytest.mark.parametrize("slots,streams,first,count", [(4, 0, 0, 4), (8, 2, 4, 4)], ids=["submit-0-4", "share-4-4-of-8"])
def test_live_update_reaches_a_cached_multi_slot_graph(blob, live, slots, streams, first, count):
    """submit(0, 4) of a 4-slot engine, and the aligned share [4, 8) of an 8-slot, 2-stream engine (the second stream's own
    graph): a submit before the set, so that the graph exists, and submits after it."""
    span = range(first, first + count)

    def step(e):
        e.submit(first, count)
        e.wait()
        return [_snap(e, s) for s in span]
    with _engine(blob, src_format=PATTERN, num_slots=slots, num_streams=streams) as be, _engine(blob, num_slots=slots, num_streams=streams) as he:
        if streams:
            assert be.num_streams == streams
        for s in span:
            be.get_src_image_buffer(s)[:] = live["raws"][s]
            he.get_src_image_buffer(s)[:] = live["base"][s]
        want_base = step(he)
        for s in span:
            he.get_src_image_buffer(s)[:] = live["isp"][s]
        want_isp = step(he)
        firsts = step(be)
        assert all(_same(x, y) for x, y in zip(firsts, want_base))
        be.set_bayer_isp(GAINS, LUT)
        assert all(_same(x, y) for x, y in zip(step(be), want_isp))
        assert all(_same(x, y) for x, y in zip(step(be), want_isp))      # the re-captured graph, replayed
        be.set_bayer_isp(UNIT)
        assert all(_same(x, y) for x, y in zip(step(be), firsts))
        assert not any(_same(x, y) for x, y in zip(want_base, want_isp))


def test_live_update_reaches_rotated_image_and_extract_armors(blob, rm_test_image):
    raw = bayer.mosaic(rm_test_image, "BGGR")
    rng = np.random.default_rng(5)
    xy0 = rng.uniform(0, 1100, (24, 2))
    boxes = np.concatenate([xy0, xy0 + rng.uniform(40, 300, (24, 2))], axis=1).astype(np.float32)
    boxes = np.concatenate([boxes, np.array([[0, 0, 1280, 1024], [300, 200, 900, 800]], np.float32)])

    def armors(e):
        out = e.extract_armors_raw(boxes)
        return bytes(out)[:len(boxes) * ctypes.sizeof(capi.Det)]

    # 255 -> (255 * 60 + 128) >> 8 = 60 -> LUT 124: nothing reaches the extraction's threshold of 150 any more, so a stale table shows
    gains = (60, 60, 60)
    assert LUT[60] < 150
    hwc0, hwc1 = bayer.demosaic(raw, "BGGR"), bayer.demosaic(raw, "BGGR", gains, lut=LUT)
    with _engine(blob, src_format="BGGR") as be, _engine(blob) as he:
        be.get_src_image_buffer()[:] = raw
        he.get_src_image_buffer()[:] = hwc0
        rot0, arm0 = be.get_rotated_image(), armors(be)
        assert np.array_equal(rot0, hwc0[::-1, ::-1]) and arm0 == armors(he)
        be.set_bayer_isp(gains, LUT)
        he.get_src_image_buffer()[:] = hwc1
        arm1 = armors(be)                                         # (the extraction first: it demosaics on its own)
        assert arm1 == armors(he) and arm1 != arm0
        assert np.array_equal(be.get_rotated_image(), hwc1[::-1, ::-1])
        be.set_bayer_isp(UNIT)
        assert np.array_equal(be.get_rotated_image(), rot0) and armors(be) == arm0


def test_a_set_between_two_async_submits_waits_for_the_first(blob, live):
    with _engine(blob, src_format=PATTERN, num_slots=2) as be, _engine(blob, num_slots=2) as he:
        he.get_src_image_buffer(0)[:] = live["base"][0]
        he.get_src_image_buffer(1)[:] = live["isp"][1]
        be.get_src_image_buffer(0)[:] = live["raws"][0]
        be.get_src_image_buffer(1)[:] = live["raws"][1]
        for e in (he, be):
            e.submit(0, 1, async_upload=True)
            if e is be:
                e.set_bayer_isp(GAINS, LUT)
            e.submit(1, 1, async_upload=True)
            e.wait()
        assert _same(_snap(be, 0), _snap(he, 0))                 # slot 0 ran with the old table: the set waited for it
        assert _same(_snap(be, 1), _snap(he, 1))
        he.get_src_image_buffer(0)[:] = live["isp"][0]
        he.detect(0)
        assert not _same(_snap(be, 0), _snap(he, 0))             # (... and the new table would have shown)


def test_setter_argument_errors_on_living_engines(blob, monkeypatch):
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    with _engine(blob, (32, 16), net_size=64) as he:
        with pytest.raises(capi.IrmvError) as ei:
            he.set_bayer_isp(UNIT)
        assert ei.value.code == capi.ERR_ARG and "IRMV_SRC_HWC8" in str(ei.value)
        with pytest.raises(capi.IrmvError):
            he.bayer_isp
    with _engine(blob, (32, 16), net_size=64, src_format="RGGB", bayer_gains=(300, 256, 256)) as be:
        with pytest.raises(capi.IrmvError) as ei:
            be.set_bayer_isp((256, 1024, 256))
        assert ei.value.code == capi.ERR_ARG and "gain_q8" in str(ei.value)
        assert be._L.irmv_engine_set_bayer_isp(be._h, None, None) == capi.ERR_ARG
        assert be.bayer_isp[0] == (300, 256, 256)                # a refused set changes nothing
        with pytest.raises(ValueError):
            be.set_bayer_isp(UNIT, np.zeros((2, 256), np.uint8))


# ---------------------------------------------------------------- the default path is today's kernel
def test_profile_names_the_demosaic_kernel_that_runs(blob, monkeypatch):
    monkeypatch.setenv("IRMV_AUTOTUNE", "0")
    monkeypatch.setenv("IRMV_GROUP_FORCE", "1")

    def names(e):
        return [k["name"] for k in e.profile(0, 1)]
    with _engine(blob) as he:
        assert not any(n.startswith("bayer_demosaic") for n in names(he))
    with _engine(blob, src_format="RGGB") as be:
        n = names(be)
        assert n[0] == "bayer_demosaic" and sum(x.startswith("bayer_demosaic") for x in n) == 1
        be.set_bayer_isp(UNIT)
        n = names(be)
        assert n[0] == "bayer_demosaic_lut" and "bayer_demosaic" not in n
    with _engine(blob, src_format="RGGB", bayer_demosaic="mhc") as me:
        n = names(me)
        assert n[0] == "bayer_demosaic_mhc" and "bayer_demosaic" not in n and sum(x.startswith("bayer_demosaic") for x in n) == 1


# ---------------------------------------------------------------- facade
def test_facade_runs_an_mhc_engine_and_sets_the_isp(tmp_path, blob):
    exe = ref.facade_exe()
    (tmp_path / "m.irmw").write_bytes(blob)
    raw = bayer.mosaic(_frame(2), "GRBG")
    raw.tofile(tmp_path / "raw.bin")
    np.ascontiguousarray(np.broadcast_to(LUT, (3, 256))).tofile(tmp_path / "lut.bin")
    out = subprocess.run([exe, str(tmp_path / "m.onnx"), str(tmp_path / "raw.bin"), str(tmp_path / "lut.bin")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr

    def lines(tag, bboxes):
        return [f"{tag} {len(bboxes)}"] + [" ".join([tag] + [float(np.float32(v)).hex() for v in (*b.xyxy, b.score)] + [str(int(b.class_id))])
                                           for b in bboxes]

    def norm(text):     # "%a" and float.hex() spell the same value differently: compare the values
        rows = []
        for ln in text.strip().splitlines():
            f = ln.split()
            rows.append((f[0],) + tuple(float.fromhex(v) for v in f[1:6]) + tuple(f[6:]) if len(f) > 2 else tuple(f))
        return rows
    with _engine(blob, src_format="GRBG", bayer_demosaic="mhc") as e:
        e.get_src_image_buffer()[:] = raw
        exp = lines("before", e.detect())
        e.set_bayer_isp(GAINS, LUT)
        exp += lines("after", e.detect())
        e.set_bayer_isp(UNIT)
        exp += lines("back", e.detect())
    assert norm(out.stdout) == norm("\n".join(exp))
