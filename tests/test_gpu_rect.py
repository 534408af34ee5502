"""Rectangular network input (irmv_engine_cfg.net_height) on the GPU, 1280 x 1024 camera frames.

References (tests/rect_ref.py, proven against the square oracle in tests/test_rect_cpu.py): the numpy restatement of the
preprocess geometry and blend, the square oracle's decode / NMS on the head embedded in a square of side max(W, H), and
tests/torch_ref.TorchNet (F.conv2d, any shape) for the network.  The per-layer check is tests/test_gpu_conv_candidates.py's
own sweep."""
import time

import numpy as np
import pytest

import rect_ref
from conftest import D_REF, K_REF
from irmv_detection_amd import arch, bayer, capi, frames, weights
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_gpu_conv_candidates import _report, load_frames, sweep
from test_gpu_engine import BOX_TOL, HEAD_TOL, KPT_TOL, SCORE_TOL, _raw_tuple
from test_gpu_light import _compare
from torch_ref import TorchNet

pytestmark = pytest.mark.gpu


def _engine(blob, W, H, **kw):
    return YoloEngine(None, (1280, 1024), weights_blob=blob, net_size=W, net_height=H, **kw)


def _stride_of(anchor, W, H):
    a0 = (W // 8) * (H // 8)
    return 8 if anchor < a0 else (16 if anchor < a0 + (W // 16) * (H // 16) else 32)


def _post_exact(e, W, H, head=None, slot=0):
    """read_raw == the embedded-square oracle on the engine's head (or on `head`, written and post-processed alone)."""
    if head is not None:
        e.write_head(head, slot)
        e.run_post(slot, 1)
    else:
        head = e.read_head(slot)
    raw, exp = e.read_raw(slot), rect_ref.decode_nms(head, W, H, 14, 8)
    assert raw["n_candidates"] == exp["n_candidates"] and raw["num_dets"] == exp["num_dets"]
    for k in ("anchors", "classes", "boxes", "scores", "kpts"):
        assert np.array_equal(raw[k], exp[k]), k
    return raw, exp


def test_dimensions_and_shapes(blob):
    with _engine(blob, 640, 512) as e:
        assert (e.net_width, e.net_height, e.net_size) == (640, 512, 640)
        assert e.num_anchors == 6720 == rect_ref.num_anchors(640, 512)
        e.detect()
        assert e.read_input(0).shape == (3, 512, 640)
        assert e.read_head(0).shape == (6720, e.head_channels)
        assert e.read_tap("15", 0).shape == (64, 80, 64) and e.read_tap("21", 0).shape == (16, 20, 256)
    with YoloEngine(None, (1280, 1024), weights_blob=blob) as e:
        assert (e.net_width, e.net_height) == (640, 640) and e.num_anchors == 8400


# ---------------------------------------------------------------- preprocess
@pytest.mark.parametrize("W,H,mode,rot,swap", [
    (640, 512, 0, True, False), (640, 512, 1, False, True), (640, 512, 0, False, True), (640, 512, 1, True, False),
    (640, 480, 0, True, False), (640, 480, 1, False, True),
    (416, 352, 1, True, False), (416, 352, 1, False, True),
    (320, 640, 0, True, True), (320, 640, 0, False, False),   # H > W: swapped axes would show
])
def test_preprocess_bit_exact(blob, W, H, mode, rot, swap):
    rng = np.random.default_rng(W + H)
    img = rng.integers(0, 256, (1024, 1280, 3), dtype=np.uint8)
    img[:512] = frames.synthetic_frame(4)[:512]
    with _engine(blob, W, H, resize_mode=mode, rotate180=rot, swap_rb=swap) as e:
        e.get_src_image_buffer(0)[:] = img
        e.detect()
        got = e.read_input(0)
        names = [st["name"] for st in e.profile(0, 1)]
    assert np.array_equal(got, rect_ref.preprocess(img, W, H, mode, rot, swap))
    assert "front_fused" in names


def test_preprocess_bit_exact_bayer(blob):
    raw = bayer.mosaic(frames.synthetic_frame(6), "RGGB")
    with _engine(blob, 640, 512, src_format="RGGB") as e:
        e.get_src_image_buffer(0)[:] = raw
        e.detect()
        got = e.read_input(0)
    assert np.array_equal(got, rect_ref.preprocess(bayer.demosaic(raw, "RGGB"), 640, 512))


# ---------------------------------------------------------------- per layer
CONFIGS = [   # (id, W, H, slots, kind)
    ("640x512x3", 640, 512, 3, "c2f"),
    ("shufflenet-int8-416x352x4", 416, 352, 4, "shuffle-int8"),
    ("320x640x2", 320, 640, 2, "c2f"),
    ("224x96x2", 224, 96, 2, "c2f"),          # odd tilings: 28 x 12 at stride 8, 14 x 6, 7 x 3
    ("2048x64x1", 2048, 64, 1, "c2f"),        # extreme aspect ratios: P5 2 x 64 and 64 x 2
    ("64x2048x1", 64, 2048, 1, "c2f"),
]


@pytest.mark.parametrize("tag,W,H,slots,kind", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_conv_candidate_is_bitwise_the_choice_and_within_the_bound(blob, capsys, tag, W, H, slots, kind):
    t0 = time.time()
    b = blob if kind == "c2f" else weights.quantize_blob_int8(weights.synthetic_blob(0, backbone=arch.BACKBONE_SHUFFLE))
    lines = []
    with _engine(b, W, H, num_slots=slots) as e:
        load_frames(e, slots)
        res = sweep(e, b, lines.append)
        for s in range(slots):
            _post_exact(e, W, H, slot=s)
        kinds = sorted({st["name"] for st in e.profile(0, 1)} & {"front_fused", "c2f2_fused", "c2f32_ab", "c2f32_a", "c2f32_b"})
    with capsys.disabled():
        print("\n".join(lines))
        print(f"[rect {tag}] fused kernels of a single-frame step: {kinds}")
    _report(tag, res, t0, capsys)


# ---------------------------------------------------------------- network
@pytest.mark.parametrize("W,H", [(640, 512), (640, 480)])
def test_head_vs_torch_reference(blob, capsys, W, H):
    tn = TorchNet(blob)
    worst = 0.0
    with _engine(blob, W, H, num_slots=8) as e:
        for s in range(8):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
        e.submit(0, 8)
        e.wait()
        for s in range(8):
            x = e.read_input(s)
            assert np.array_equal(x, rect_ref.preprocess(frames.synthetic_frame(s), W, H))
            ref = tn.forward(x).numpy()
            err = float(np.abs(e.read_head(s) - ref).max())
            worst = max(worst, err)
            assert err <= HEAD_TOL, (s, err)
    with capsys.disabled():
        print(f"\n[rect {W}x{H}] head max|d| vs TorchNet over frames 0..7: {worst:.4f} (tolerance {HEAD_TOL})")


# ---------------------------------------------------------------- decode / NMS / keypoints
def _crowded_head(rng, A, hot):
    head = np.zeros((A, 86), np.float32)
    head[:, :64] = rng.standard_normal((A, 64)) - 0.4 * (np.arange(64) % 16)
    cls = rng.standard_normal((A, 14)) - 6.0
    m = rng.random((A, 14)) < hot
    cls[m] = rng.uniform(-1.0, 4.0, m.sum())
    head[:, 64:78] = cls
    head[:, 78:] = 0.25 + 0.3 * rng.standard_normal((A, 8))
    return head


@pytest.mark.parametrize("W,H", [(640, 512), (416, 352), (1568, 1568), (2048, 2048), (2048, 1216)])   # up to 86016 anchors
def test_post_exact_on_engine_and_synthetic_heads(blob, W, H):
    with _engine(blob, W, H, num_slots=2) as e:
        for fi in (0, 1, 2):
            e.get_src_image_buffer(0)[:] = frames.synthetic_frame(fi)
            e.detect(0)
            raw, _ = _post_exact(e, W, H)
            assert raw["num_dets"] > 0
        A = rect_ref.num_anchors(W, H)
        for hot in (0.0, 0.00002, 0.004, 0.008, 0.03):
            rng = np.random.default_rng(int(hot * 1e6) + W)
            raw, _ = _post_exact(e, W, H, _crowded_head(rng, A, hot), slot=1)
            if hot == 0.03:
                assert raw["n_candidates"] > 1024
        # the last anchor of every level carries the top score: level boundaries and the last record are read
        head = _crowded_head(np.random.default_rng(9), A, 0.0)
        head[:, 64:78] = -20.0
        base = 0
        for s in (8, 16, 32):
            base += (W // s) * (H // s)
            head[base - 1, 64 + s % 14] = 6.0
        raw, _ = _post_exact(e, W, H, head, slot=1)
        assert raw["num_dets"] == 3


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("mode", [capi.RESIZE_STRETCH, capi.RESIZE_LETTERBOX])
def test_detect_end_to_end(blob, mode):
    W, H = 640, 512
    tn = TorchNet(blob)
    nw, nh, px, py = rect_ref.geometry(1280, 1024, W, H, mode)
    compared = 0
    with _engine(blob, W, H, resize_mode=mode) as e:
        for fi in (0, 3):
            frame = frames.synthetic_frame(fi)
            e.get_src_image_buffer(0)[:] = frame
            armors = e.detect_armors(0)
            raw = e.read_raw(0)
            # what detect() returns == the embedded oracle on the engine's own head, mapped per axis
            own = rect_ref.decode_nms(e.read_head(0), W, H, 14, 8)
            assert raw["num_dets"] == own["num_dets"] == len(armors) > 0
            xy = rect_ref.parse_output(own["boxes"], 1280, 1024, W, H, mode)
            assert np.array_equal(np.array([a.bbox_xyxy for a in armors], np.float32), xy)
            kp = own["kpts"].reshape(-1, 4, 2)
            kp_src = np.stack([(kp[..., 0] - np.float32(px)) * (np.float32(1280) / np.float32(nw)),
                               (kp[..., 1] - np.float32(py)) * (np.float32(1024) / np.float32(nh))], -1).reshape(-1, 8)
            for a, k in zip(armors, kp_src):
                got = np.array([*a.left_light.bottom, *a.left_light.top, *a.right_light.top, *a.right_light.bottom], np.float32)
                assert np.abs(got - k).max() <= 1e-3
                o = oracle.solve_pnp_ippe(K_REF, D_REF, a.image_points(), 0)
                assert o["ok"] == a.pnp_ok
                if a.pnp_ok:
                    assert np.abs(o["rvec"] - a.rvec).max() <= 1e-6 and np.abs(o["tvec"] - a.tvec).max() <= 1e-6
            # against the fp32 reference head end to end: the shared survivors agree up to fp16 noise
            ref = rect_ref.decode_nms(tn.forward(rect_ref.preprocess(frame, W, H, mode)).numpy(), W, H, 14, 8)
            got = {(int(a), int(c)): i for i, (a, c) in enumerate(zip(raw["anchors"], raw["classes"]))}
            want = {(int(a), int(c)): i for i, (a, c) in enumerate(zip(ref["anchors"], ref["classes"]))}
            common = set(got) & set(want)
            assert len(common) >= 0.9 * max(len(want), 1)
            ref_src = rect_ref.parse_output(ref["boxes"], 1280, 1024, W, H, mode)
            for k in common:
                st = _stride_of(k[0], W, H)
                assert np.abs(raw["boxes"][got[k]] - ref["boxes"][want[k]]).max() <= BOX_TOL(st)
                assert np.abs(xy[got[k]] - ref_src[want[k]]).max() <= 2 * BOX_TOL(st)      # 2 source pixels per net pixel
                assert abs(raw["scores"][got[k]] - ref["scores"][want[k]]) <= SCORE_TOL
                assert np.abs(raw["kpts"][got[k]] - ref["kpts"][want[k]]).max() <= KPT_TOL
            compared += len(common)
    assert compared > 0


def test_classical_points(blob):
    with _engine(blob, 640, 512, point_source=capi.POINTS_CLASSICAL, num_slots=2) as e:
        n_valid = 0
        for s in range(2):
            e.get_src_image_buffer(s)[:] = frames.synthetic_frame(s)
        e.submit(0, 2)
        e.wait()
        for s in range(2):
            arm = e.results(s)
            assert len(arm) > 0
            n_valid += _compare(arm, oracle.rotate180(frames.synthetic_frame(s)), np.array([a.bbox_xyxy for a in arm], np.float32))
        assert n_valid > 0


# ---------------------------------------------------------------- shapes of the step
def test_batched_step_equals_per_slot_detect(blob):
    imgs = [frames.synthetic_frame(20 + i) for i in range(6)]
    with _engine(blob, 640, 512, num_slots=6, num_streams=2) as e:
        single = []
        for s, im in enumerate(imgs):
            e.get_src_image_buffer(s)[:] = im
            e.detect(s)
            single.append((e.read_head(s).copy(), _raw_tuple(e.read_raw(s))))
        e.submit(0, 6)
        e.wait()
        for s in range(6):
            assert np.array_equal(e.read_head(s), single[s][0]), s
            r = _raw_tuple(e.read_raw(s))
            assert r[0] == single[s][1][0] and all(np.array_equal(a, b) for a, b in zip(r[1:], single[s][1][1:])), s
    assert not np.array_equal(single[0][0], single[1][0])


@pytest.mark.parametrize("slots,count", [(1, 1), (3, 1), (8, 4)])
def test_launch_list_is_that_of_the_square_engine(blob, monkeypatch, capsys, slots, count):
    """The same launches in the same order at 640 x 512 as at 640 x 640: no fused kernel declines the rectangle.
    (IRMV_GROUP_FORCE=1: the grouped Detect launches are kept whatever their timing says, on both engines.)"""
    monkeypatch.setenv("IRMV_GROUP_FORCE", "1")
    lists = {}
    for H in (640, 512):
        with _engine(blob, 640, H, num_slots=slots) as e:
            lists[H] = e.profile(0, count)
    layers = {H: [st["layer"] for st in v] for H, v in lists.items()}
    assert layers[512] == layers[640]
    fused = ("front_fused", "c2f2_fused", "c2f32_", "bneck64_", "kpt3_", "+1x1", "head_")
    kinds = {H: sorted({f for st in v for f in fused if f in st["name"]}) for H, v in lists.items()}
    assert kinds[512] == kinds[640]
    assert {"front_fused", "c2f2_fused", "c2f32_", "+1x1"} <= set(kinds[512])
    with capsys.disabled():
        print(f"\n[rect launch list {slots} slots, {count} per step] {len(layers[512])} launches, layers identical to 640 x 640; fused: {kinds[512]}")


def test_net_height_equal_to_net_size_is_the_square_engine(blob):
    out = {}
    for H in (None, 640):
        with _engine(blob, 640, H, num_slots=2) as e:
            for s in range(2):
                e.get_src_image_buffer(s)[:] = frames.synthetic_frame(30 + s)
            e.submit(0, 2)
            e.wait()
            out[H] = [(e.read_head(s).copy(), _raw_tuple(e.read_raw(s))) for s in range(2)]
            e.detect(0)
            out[H].append((e.read_head(0).copy(), _raw_tuple(e.read_raw(0))))
    for (ha, ra), (hb, rb) in zip(out[None], out[640]):
        assert np.array_equal(ha, hb)
        assert ra[0] == rb[0] and all(np.array_equal(a, b) for a, b in zip(ra[1:], rb[1:]))


# ---------------------------------------------------------------- every bitwise switch at 640 x 512
SWITCHES = ["IRMV_INLINE_COPIES=1", "IRMV_ZERO_COPY_RESULTS=0", "IRMV_SPLIT_SCAN=0", "IRMV_EMIT_SCAN=0",
            "IRMV_FUSED_HEAD=0", "IRMV_MERGE_HEAD0=0", "IRMV_GROUP_HEAD=0", "IRMV_NO_PF2=1", "IRMV_NO_DEEP=1",
            "IRMV_FRONT_FASTX=0", "IRMV_FRONT_DIRECT=0", "IRMV_FRONT_TILE8=0",
            "IRMV_STREAMS=1", "IRMV_AUTOTUNE=0", "IRMV_GROUP_FORCE=1", "IRMV_NUMA=0", "IRMV_GRAPH_UPLOAD=0", "IRMV_XCD_IMAGES=0",
            "IRMV_NO_NT8=1", "IRMV_NMS_CLASSWALK=0", "IRMV_NO_PF4=1", "IRMV_WRES_STAGGER=0", "IRMV_BNECK64=0", "IRMV_KPT3=0",
            "IRMV_UPLOAD_KERNEL=0", "IRMV_SYNC_LAUNCH=graph", "IRMV_SYNC_LAUNCH=eager",
            "IRMV_FUSED_FRONT=0", "IRMV_FUSED_C2F=0"]    # (the fused kernels' switches: tests/test_gpu_engine.py test_fused_kernels_*)


@pytest.mark.parametrize("switch", SWITCHES)
def test_every_switch_is_bitwise_the_default(blob, monkeypatch, switch):
    imgs = [frames.synthetic_frame(120 + i) for i in range(4)]

    def run():
        out = []
        for slots in (4, 1):
            with _engine(blob, 640, 512, num_slots=slots) as e:
                for s in range(slots):
                    e.get_src_image_buffer(s)[:] = imgs[s]
                e.submit(0, slots); e.wait()
                out += [e.read_head(s).copy() for s in range(slots)]
                out += [_raw_tuple(e.read_raw(s)) for s in range(slots)]
                for s in range(slots):
                    e.submit(s, 1, async_upload=True)
                for s in range(slots):
                    e.wait_slots(s, 1)
                out += [_raw_tuple(e.read_raw(s)) for s in range(slots)]
                e.detect(0)
                out.append(_raw_tuple(e.read_raw(0)))
                out += [e.read_input(0).copy(), e.read_tap("1", 0).copy(), e.read_tap("2", 0).copy()]
        return out

    name, val = switch.split("=")
    monkeypatch.delenv(name, raising=False)
    want = run()
    monkeypatch.setenv(name, val)
    got = run()
    assert len(want) == len(got)
    for a, b in zip(want, got):
        if isinstance(a, tuple):
            assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), switch
        else:
            assert np.array_equal(a, b), switch
