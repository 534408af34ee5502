"""Sparse Detect head: a step stores the head rows of candidate anchors only (class carriers set a bit per candidate anchor,
box carriers and the keypoint launch store where it is set, nms_pnp_kernel clears the bitmap).  Everything a caller can
observe -- detections, candidate counts, the head read back -- must be what the dense stores (IRMV_SPARSE_HEAD=0) give,
bit for bit.  The variable is read at engine creation, so every comparison builds separate engines."""
import numpy as np
import pytest

from irmv_detection_amd import capi, frames
from irmv_detection_amd.engine import YoloEngine
from oracle import oracle
from test_gpu_engine import _assert_post_exact, _clustered_head, _load, _raw_tuple, _synthetic_head

pytestmark = pytest.mark.gpu


def _same_raw(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def _det_tuple(e, slot):
    return [(int(d.armor_class), d.confidence, d.bbox_xyxy) for d in e.results(slot)]


def _bits_clear(e, slots):
    for s in range(slots):
        sparse, words = e.debug_cand_bits(s)
        assert sparse and len(words) == (e.num_anchors + 31) // 32
        assert not words.any(), (s, np.nonzero(words)[0][:8])


def _run_frames(blob, monkeypatch, slots, imgs, sparse):
    """Per frame: (raw tuple, n_candidates, detections, head read back, raw tuple of a second step after the read-back)."""
    if sparse:
        monkeypatch.delenv("IRMV_SPARSE_HEAD", raising=False)
    else:
        monkeypatch.setenv("IRMV_SPARSE_HEAD", "0")
    out = []
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=slots) as e:
        assert e.debug_cand_bits(0)[0] == sparse
        for f0 in range(0, len(imgs), slots):
            n = min(slots, len(imgs) - f0)
            for s in range(n):
                _load(e, s, imgs[f0 + s])
            e.submit(0, n); e.wait()
            if sparse:
                _bits_clear(e, slots)
            first = [(_raw_tuple(e.read_raw(s)), e.read_raw(s)["n_candidates"], _det_tuple(e, s)) for s in range(n)]
            heads = [e.read_head(s).copy() for s in range(n)]
            e.submit(0, n); e.wait()       # the read-back must leave no bit set and no row stale
            if sparse:
                _bits_clear(e, slots)
            for s in range(n):
                out.append(first[s] + (heads[s], _raw_tuple(e.read_raw(s))))
    return out


@pytest.mark.parametrize("slots", [8, 1])
def test_sparse_head_is_bitwise_the_dense_head(blob, rm_test_image, monkeypatch, slots):
    """Synthetic frames 0 .. 15 and rm_test.jpg through a batched engine (8 slots, two streams) and a single-slot engine:
    raw outputs, candidate counts, detections and the head read back are those of the dense engine; a second step after the
    read-back repeats the first; the bitmap is all zero after every step."""
    imgs = [frames.synthetic_frame(i) for i in range(16)] + [rm_test_image]
    assert imgs[-1].shape == (1024, 1280, 3)
    want = _run_frames(blob, monkeypatch, slots, imgs, False)
    got = _run_frames(blob, monkeypatch, slots, imgs, True)
    assert len(want) == len(got) == 17
    some = 0
    for i, (w, g) in enumerate(zip(want, got)):
        assert _same_raw(w[0], g[0]), i
        assert w[1] == g[1], (i, w[1], g[1])
        assert w[2] == g[2], i
        assert np.array_equal(w[3], g[3]), (i, np.nonzero((w[3] != g[3]).any(1))[0][:8], np.nonzero((w[3] != g[3]).any(0))[0][:8])
        assert _same_raw(g[0], g[4]) and _same_raw(w[0], w[4]), i
        some += w[1] > 0
    assert some >= 10       # nothing vacuous: most frames have candidates


def test_frames_without_a_candidate(blob, monkeypatch):
    """An all-zero image, and a threshold no logit reaches: no key, no bit, no detection -- and the head read back is still
    the dense engine's."""
    heads = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("IRMV_SPARSE_HEAD")
        else:
            monkeypatch.setenv("IRMV_SPARSE_HEAD", mode)
        with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=2, score_thr=0.999999) as e:
            _load(e, 0, np.zeros((1024, 1280, 3), np.uint8))
            _load(e, 1, frames.synthetic_frame(3))
            e.submit(0, 2); e.wait()
            for s in range(2):
                raw = e.read_raw(s)
                assert raw["n_candidates"] == 0 and raw["num_dets"] == 0
            if mode is None:
                _bits_clear(e, 2)
            heads[mode] = [e.read_head(s).copy() for s in range(2)]
    for a, b in zip(heads["0"], heads[None]):
        assert np.array_equal(a, b)


def test_host_written_heads_keep_their_paths(blob):
    """write_head / run_post on an engine with the sparse head: a written head is not stale (nothing re-computes it), the
    crowded heads of the NMS tests (> 512 and > 8192 candidates) pass through run_post against the oracle, also right
    after a step on the same slot."""
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=2) as e:
        assert e.debug_cand_bits(0)[0]
        _load(e, 0, frames.synthetic_frame(5)); _load(e, 1, frames.synthetic_frame(6))
        e.submit(0, 2); e.wait()
        raw = _assert_post_exact(e, _clustered_head(np.random.default_rng(5), 1600, 600))       # start-over path
        assert raw["n_candidates"] > 1600
        head = _synthetic_head(np.random.default_rng(21), 0.15)
        raw = _assert_post_exact(e, head)
        assert raw["n_candidates"] > capi.CAND_CAP
        assert np.array_equal(e.read_head(0), head)        # as written: the read-back step did not run over it
        _bits_clear(e, 2)
        e.submit(0, 2); e.wait()                           # a step on a slot whose head was host-written
        _bits_clear(e, 2)
        raw = _assert_post_exact(e, _clustered_head(np.random.default_rng(7), 700, 300), slot=1)
        assert raw["n_candidates"] > 512


@pytest.mark.parametrize("slots", [4, 1])
def test_run_post_after_a_step_gives_the_steps_detections(blob, slots):
    """step; run_post on the same slot: run_post's scan reads every anchor's class logits, so the slot's head is first brought
    to the dense state -- the detections are the step's own, and the oracle's on the head read back."""
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=slots) as e:
        for s in range(slots):
            _load(e, s, frames.synthetic_frame(40 + s))
        e.submit(0, slots); e.wait()
        step = [_raw_tuple(e.read_raw(s)) for s in range(slots)]
        ncand = [e.read_raw(s)["n_candidates"] for s in range(slots)]
        assert max(ncand) > 0
        e.run_post(0, slots)
        for s in range(slots):
            raw = e.read_raw(s)
            assert _same_raw(step[s], _raw_tuple(raw)) and raw["n_candidates"] == ncand[s], s
        _bits_clear(e, slots)
        hd = e.read_head(slots - 1)
        exp = oracle.decode_nms(hd, 640, 14, 8)
        raw = e.read_raw(slots - 1)
        assert raw["n_candidates"] == exp["n_candidates"] and raw["num_dets"] == exp["num_dets"]
        assert np.array_equal(raw["anchors"], exp["anchors"]) and np.array_equal(raw["boxes"], exp["boxes"])
        assert np.array_equal(raw["scores"], exp["scores"]) and np.array_equal(raw["kpts"], exp["kpts"])


def test_crowded_camera_crop_through_a_sparse_step(blob):
    """The 4 900-candidate camera crop of the NMS tests as a whole step (more than half of the anchors are candidates; > 512:
    the first-walk path): against the oracle on the head read back."""
    with YoloEngine(None, (640, 640), weights_blob=blob) as e:
        assert e.debug_cand_bits(0)[0]
        _load(e, 0, np.ascontiguousarray(frames.synthetic_frame(1)[:640, :640]))
        e.detect(0)
        raw, hd = e.read_raw(0), e.read_head(0)
        exp = oracle.decode_nms(hd, 640, 14, 8)
        assert raw["n_candidates"] == exp["n_candidates"] > 4000
        assert raw["num_dets"] == exp["num_dets"] and np.array_equal(raw["anchors"], exp["anchors"]) and np.array_equal(raw["boxes"], exp["boxes"])
        assert np.array_equal(raw["scores"], exp["scores"]) and np.array_equal(raw["kpts"], exp["kpts"])
        _bits_clear(e, 1)
