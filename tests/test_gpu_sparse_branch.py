"""Sparse branch: behind the class carriers the Detect box branch (first conv with a one-pixel halo, carriers) and the keypoint
launch skip every (tile, image) pair without a candidate anchor (ConvArgs::tile_gate, Kpt3Args::tile_gate).  Only fewer tiles
are visited: everything a caller can observe is what an engine created with IRMV_SPARSE_BRANCH=0 gives, bit for bit.  The
variable is read at engine creation, so every comparison builds separate engines; a reference run is computed once per
configuration and shared.

What no test here shows is that a skip HAPPENS: stores are gated per anchor with or without the tile gate, the read-backs run
the layers densely, and the library has no entry that copies an activation tensor without a read-back in front (one more
debug entry only for this was left out on purpose).  A kernel that ignores the gate is a correct implementation; that the
gated ones skip is a matter of the per-launch times under profiles/ (sparse_branch_ab.txt).  The tests assert the plan side:
the gated launches stand behind the class carriers."""
import numpy as np
import pytest

from irmv_detection_amd import frames
from irmv_detection_amd.engine import YoloEngine
from test_gpu_engine import _load, _raw_tuple

pytestmark = pytest.mark.gpu

# tile shapes (rows, columns) of the gated kernels, as the kernels have them
KPT_TILE = (10, 10)      # k_kpt.hip KT: every level
PP_TILE = (8, 16)        # k_conv.hip, resident weights, ping-pong: NWP 4 waves x MT 2 x (16 >> twc_log2 = 1) rows, TWc 16 columns
LOCK_TILE = (16, 16)     # ... lockstep on a 2-D block: NWP 8
RUN_PX = 256             # ... lockstep on a row run: 16 x NWP 8 x MT 2 consecutive anchors
TAPS = ("22.cv2.0.0", "22.cv2.1.0", "22.cv2.2.0")
HIGH_THR = 0.9           # (CPU oracle: frames 3 and 14 keep ONE candidate, frame 11 none, frame 0 has 45 / 12 / 4 per level)
# frame 100 has no candidate at all (0.25), frame 3 none on the coarsest level: both inside a full batch, beside frames that have some
ORDER = list(range(9)) + [100] + list(range(9, 16)) + ["rm"]

_ref = {}


def _images(rm_test_image):
    return [rm_test_image if f == "rm" else frames.synthetic_frame(f) for f in ORDER]


def _logit_thr(thr):
    t = np.float64(np.float32(thr))
    return np.float32(np.log(t / (1.0 - t)))


def _same_raw(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def _run(blob, monkeypatch, imgs, branch, slots, thr, net=640, streams=None, wres=None):
    """Per frame: raw tuple, n_candidates, detections, head read back, the three box-branch first convs read back, raw tuple of
    a second step after the read-backs.  Plus the layers of a step's launches in order."""
    key = (branch, slots, thr, net, streams, wres, len(imgs))
    if not branch and key in _ref:
        return _ref[key]
    monkeypatch.delenv("IRMV_SPARSE_HEAD", raising=False)
    for v, val in (("IRMV_SPARSE_BRANCH", None if branch else "0"), ("IRMV_FORCE_WRES", wres)):
        if val is None:
            monkeypatch.delenv(v, raising=False)
        else:
            monkeypatch.setenv(v, val)
    kw = {} if streams is None else dict(num_streams=streams)
    out = []
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=slots, score_thr=thr, net_size=net, **kw) as e:
        assert e.debug_cand_bits(0)[0]
        for f0 in range(0, len(imgs), slots):
            n = min(slots, len(imgs) - f0)
            for s in range(n):
                _load(e, s, imgs[f0 + s])
            e.submit(0, n); e.wait()
            for s in range(slots):
                assert not e.debug_cand_bits(s)[1].any(), s
            first = [(_raw_tuple(e.read_raw(s)), e.read_raw(s)["n_candidates"], [(int(d.armor_class), d.confidence, d.bbox_xyxy) for d in e.results(s)]) for s in range(n)]
            heads = [e.read_head(s).copy() for s in range(n)]
            taps = [[e.read_tap(t, s).copy() for t in TAPS] for s in range(n)]
            e.submit(0, n); e.wait()       # the read-backs left nothing stale and no bit set: the step repeats itself
            for s in range(slots):
                assert not e.debug_cand_bits(s)[1].any(), s
            for s in range(n):
                out.append(first[s] + (heads[s], taps[s], _raw_tuple(e.read_raw(s))))
        prof = e.profile(0, slots) if slots > 1 else []
        plan = [(st["layer"], st["name"]) for st in prof]
    res = (out, plan, None)
    if not branch:
        _ref[key] = res
    return res


def _compare(want, got):
    assert len(want) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        assert _same_raw(w[0], g[0]), i
        assert w[1] == g[1], (i, w[1], g[1])
        assert w[2] == g[2], i
        assert np.array_equal(w[3], g[3]), (i, np.nonzero((w[3] != g[3]).any(1))[0][:8], np.nonzero((w[3] != g[3]).any(0))[0][:8])
        for t, a, b in zip(TAPS, w[4], g[4]):
            assert np.array_equal(a, b), (i, t, np.argwhere((a != b).any(-1))[:4])
        assert _same_raw(g[0], g[5]) and _same_raw(w[0], w[5]), i


def _gated_plan(plan, first_convs):
    """The gated engine's step: the listed box-branch first convs and every box carrier stand behind the last class carrier."""
    layers = [l for l, _ in plan]
    last_cls = max(i for i, l in enumerate(layers) if l.startswith("model.22.cv3.") and l.endswith(".1"))
    for l in first_convs:
        assert layers.index(l) > last_cls, (l, layers)
    for lv in range(3):
        assert layers.index(f"model.22.cv2.{lv}.1") > last_cls, layers


def _levels(net):
    base, out = 0, []
    for s in (8, 16, 32):
        n = net // s
        out.append((base, n, n))
        base += n * n
    return out


def _cand_maps(recs, thr, net, nc=14):
    """[frame][level] -> bool [H, W]: the candidate anchors of the dense engine's head."""
    lt = _logit_thr(thr)
    return [[(r[3][b:b + h * w, 64:64 + nc] > lt).any(1).reshape(h, w) for b, h, w in _levels(net)] for r in recs]


def _tile_activity(m, th, tw):
    H, W = m.shape
    ny, nx = -(-H // th), -(-W // tw)
    p = np.zeros((ny * th, nx * tw), bool)
    p[:H, :W] = m
    return p.reshape(ny, th, nx, tw).any(axis=(1, 3))


def _assert_not_vacuous(maps, slots, streams, tiles, runs_and_images=True):
    """tiles: (level, rows, columns) of the gated kernels' 2-D tiles; runs_and_images: also the row runs of RUN_PX anchors on
    levels 1 and 2 and the images of a launch."""
    for lv, th, tw in tiles:
        ys, xs = np.nonzero(np.stack([m[lv] for m in maps]).any(0))
        H, W = maps[0][lv].shape
        last_y = np.minimum(ys // th * th + th - 1, H - 1) == ys
        last_x = np.minimum(xs // tw * tw + tw - 1, W - 1) == xs
        assert (ys % th == 0).any() and last_y.any() and (xs % tw == 0).any() and last_x.any(), (lv, th, tw)
        adj = False     # an inactive (tile, image) pair beside an active one, in the image and along the images of a workgroup
        for m in maps:
            a = _tile_activity(m[lv], th, tw)
            adj = adj or (a[:, 1:] != a[:, :-1]).any() or (a[1:] != a[:-1]).any()
        assert adj, (lv, th, tw)
    if not runs_and_images:
        return
    for lv in (1, 2):   # row runs under halo 0 (box carriers): a candidate AT a run's first and at a run's last anchor
        idx = np.nonzero(np.stack([m[lv].reshape(-1) for m in maps]).any(0))[0]
        assert ((idx % RUN_PX == 0) & (idx >= RUN_PX)).any() and (idx % RUN_PX == RUN_PX - 1).any(), lv
    share = -(-slots // streams)
    beside = [False, False, False]   # an image without a candidate on a level next to one that has some, in the same launch
    for f0 in range(0, len(maps), slots):
        for s in range(min(slots, len(maps) - f0) - 1):
            if s // share == (s + 1) // share:
                for lv in range(3):
                    beside[lv] = beside[lv] or (maps[f0 + s][lv].any() != maps[f0 + s + 1][lv].any())
    assert all(beside), beside


@pytest.mark.parametrize("slots,thr", [(8, 0.25), (8, HIGH_THR), (3, 0.25), (3, HIGH_THR)])
def test_whole_steps_at_the_benchmarked_size(blob, rm_test_image, monkeypatch, slots, thr):
    """640 x 640 net, 1280 x 1024 frames, two streams, the resident-weight kernels the benchmark's tile table picks selected with
    IRMV_FORCE_WRES=3: level 0's box branch on the 80 x 80 ping-pong form, the other levels' carriers in lockstep on row runs
    (8 slots: four per stream, image groups of three and one; 3 slots: two and one, so the ping-pong groups' lists are short,
    odd and unequal).  Frames 0 .. 15, 100 and rm_test.jpg
    at score_thr 0.25 and at 0.9, which leaves isolated candidates: raw outputs, candidate counts, detections, the head and the
    three first convs read back, a second step after the read-backs and the cleared bitmap against IRMV_SPARSE_BRANCH=0."""
    imgs = _images(rm_test_image)
    want, _, _ = _run(blob, monkeypatch, imgs, False, slots, thr, streams=2, wres="3")
    got, plan, _ = _run(blob, monkeypatch, imgs, True, slots, thr, streams=2, wres="3")
    _compare(want, got)
    names = dict(plan)
    assert "_wres_pp" in names["model.22.cv2.0.0"] and "_wres_pp" in names["model.22.cv2.0.1"], names
    assert "_wres" in names["model.22.cv2.1.1"] and "_wres" in names["model.22.cv2.2.1"], names
    _gated_plan(plan, ["model.22.cv2.0.0"])
    assert sum(w[1] > 0 for w in want) >= (14 if thr == 0.25 else 10)


def test_the_frame_set_reaches_the_gates_edges(blob, rm_test_image, monkeypatch):
    """Nothing vacuous, from the dense engine's heads: candidates in the first and the last row and
    column of each gated kernel's tile, inactive (tile, image) pairs next to active ones, and on every level an image without
    a candidate beside one that has some inside one launch."""
    imgs = _images(rm_test_image)
    maps = []
    for thr in (0.25, HIGH_THR):
        want, _, _ = _run(blob, monkeypatch, imgs, False, 8, thr, streams=2, wres="3")
        m = _cand_maps(want, thr, 640)
        if thr == 0.25:     # (the candidates of the high threshold are a subset of these)
            assert not any(x.any() for x in m[ORDER.index(100)])
            _assert_not_vacuous(m, 8, 2, [(0,) + KPT_TILE, (1,) + KPT_TILE, (2,) + KPT_TILE, (0,) + PP_TILE])
        maps.append(m)
    assert min(int(sum(x.sum() for x in f)) for f in maps[1] if any(x.any() for x in f)) <= 2    # isolated candidates at the high threshold
    assert not maps[0][ORDER.index(3)][2].any() and maps[0][ORDER.index(2)][2].any()


def test_rows_as_the_step_left_them(blob, monkeypatch):
    """A sentinel in every head row, a step on frames A, a step on other frames B, then the head as it lies in memory: at B's
    candidate anchors the box and keypoint channels are B's dense rows bit for bit; at A's candidate anchors that are none of
    B's they are still A's; every other row (and every class channel: the class carriers store none) is still the sentinel.
    A tile wrongly skipped for B shows A's row or the sentinel where B's belongs."""
    A = [frames.synthetic_frame(i) for i in range(8)]
    B = [frames.synthetic_frame(8 + i) for i in range(8)]
    SENT = np.float32(-1234.5)
    lt = _logit_thr(0.25)
    raws = {}
    for branch in (False, True):
        if branch:
            monkeypatch.delenv("IRMV_SPARSE_BRANCH", raising=False)
        else:
            monkeypatch.setenv("IRMV_SPARSE_BRANCH", "0")
        with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=8) as e:
            for s in range(8):
                _load(e, s, A[s])
            e.submit(0, 8); e.wait()
            dense_a = [e.read_head(s).copy() for s in range(8)]
            sent = np.full((e.num_anchors, e.head_channels), SENT, np.float32)
            for s in range(8):
                e.write_head(sent, s)
            e.submit(0, 8); e.wait()
            for s in range(8):
                _load(e, s, B[s])
            e.submit(0, 8); e.wait()
            raw = [e.debug_read_head_raw(s).copy() for s in range(8)]
            assert all(np.array_equal(r, e.debug_read_head_raw(s)) for s, r in enumerate(raw))     # (reads nothing into being)
            dense_b = [e.read_head(s).copy() for s in range(8)]
        raws[branch] = (raw, dense_b)
        total = only_a = 0
        for s in range(8):
            cand_a, cand_b = ((d[:, 64:78] > lt).any(1) for d in (dense_a[s], dense_b[s]))
            total += int(cand_b.sum())
            only_a += int((cand_a & ~cand_b).sum())
            rest, want_a, want_b = (np.concatenate([x[:, :64], x[:, 78:]], 1) for x in (raw[s], dense_a[s], dense_b[s]))
            assert np.array_equal(rest[cand_b], want_b[cand_b]), (branch, s, np.nonzero((rest != want_b).any(1) & cand_b)[0][:8])
            old = cand_a & ~cand_b
            assert np.array_equal(rest[old], want_a[old]), (branch, s, np.nonzero((rest != want_a).any(1) & old)[0][:8])
            none = ~(cand_a | cand_b)
            assert (rest[none] == SENT).all(), (branch, s, np.nonzero((rest != SENT).any(1) & none)[0][:8])
            assert (raw[s][:, 64:78] == SENT).all(), (branch, s)
        assert total > 400 and only_a > 100
    for s in range(8):
        assert np.array_equal(raws[False][0][s], raws[True][0][s]) and np.array_equal(raws[False][1][s], raws[True][1][s]), s


@pytest.mark.parametrize("net,slots,wres", [(320, 2, "2"), (320, 5, "2"), (640, 3, "-3")])
def test_the_other_resident_weight_forms(blob, rm_test_image, monkeypatch, net, slots, wres):
    """IRMV_FORCE_WRES on one stream.  A 320 net: 40 x 40 / 20 x 20 / 10 x 10 levels, level 0's first conv (halo 1) and all three
    box carriers in lockstep on row runs, image groups of two with a short last one at 5 slots.  640 with -3: level 0 in
    lockstep on 16 x 16 blocks.  The comparisons of the benchmarked size."""
    imgs = _images(rm_test_image)
    if net == 640:
        imgs = imgs[:10]           # frames 0 .. 8 and 100
    want, _, _ = _run(blob, monkeypatch, imgs, False, slots, 0.25, net=net, streams=1, wres=wres)
    got, plan, _ = _run(blob, monkeypatch, imgs, True, slots, 0.25, net=net, streams=1, wres=wres)
    _compare(want, got)
    names = dict(plan)
    for l in ("model.22.cv2.0.0", "model.22.cv2.0.1", "model.22.cv2.1.1", "model.22.cv2.2.1"):
        assert "_wres" in names[l] and "_pp" not in names[l], (l, names[l])
    _gated_plan(plan, ["model.22.cv2.0.0"])
    maps = _cand_maps(want, 0.25, net)
    assert sum(any(x.any() for x in f) for f in maps) >= len(imgs) // 2
    if net == 640:
        _assert_not_vacuous(maps, slots, 1, [(0,) + LOCK_TILE], runs_and_images=False)
    else:           # row runs of 256 anchors on a 40 x 40 map: runs that hold a candidate next to runs that hold none
        act = np.stack([[f[0].reshape(-1)[k:k + RUN_PX].any() for k in range(0, 1600, RUN_PX)] for f in maps])
        assert (act[:, 1:] != act[:, :-1]).any() and (act[1:] != act[:-1]).any()
        # the halo's reach on a row run (the first conv's run grows by a row and a pixel each way): a candidate within Wout + 1
        # anchors of a run's end whose NEXT run holds none, and one as close to a run's start whose PREVIOUS run holds none --
        # those neighbours are computed only because of the halo, and the candidate's box row needs them
        W, fwd, back = 40, False, False
        for f, a in zip(maps, act):
            for i in np.nonzero(f[0].reshape(-1))[0]:
                r, o = divmod(int(i), RUN_PX)
                fwd = fwd or (o >= RUN_PX - 1 - W and r + 1 < len(a) and not a[r + 1])
                back = back or (o <= W and r > 0 and not a[r - 1])
        assert fwd and back


def test_the_switch_and_single_frame_engines(blob, monkeypatch):
    """IRMV_SPARSE_BRANCH=0 and a single-slot engine keep the box branch's first conv in front of the class carriers (nothing
    is gated: a grouped head launch has no order to gate on)."""
    for env, slots in (("0", 4), (None, 1)):
        if env is None:
            monkeypatch.delenv("IRMV_SPARSE_BRANCH", raising=False)
        else:
            monkeypatch.setenv("IRMV_SPARSE_BRANCH", env)
        with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=slots, num_streams=min(slots, 2)) as e:
            _load(e, 0, frames.synthetic_frame(1))
            layers = [st["layer"] for st in e.profile(0, slots)]
            first = [i for i, l in enumerate(layers) if l.startswith("model.22.cv2.0.0") or l.startswith("model.22.s0.0")]
            later = [i for i, l in enumerate(layers) if l.startswith(("model.22.cv3.", "model.22.cv2.0.1"))]    # (a grouped launch is listed under its first member)
            assert first and later and first[0] < min(later), layers


def test_read_tap_of_the_first_conv_runs_the_read_back_only_when_stale(blob):
    """After a gated step read_tap of 22.cv2.0.0 runs the read-back step; once the slot is no longer stale a second read runs
    nothing: a head stored with write_head in between stays as written."""
    with YoloEngine(None, (1280, 1024), weights_blob=blob, num_slots=4, num_streams=2) as e:
        for s in range(4):
            _load(e, s, frames.synthetic_frame(20 + s))
        e.submit(0, 4); e.wait()
        first = e.read_tap(TAPS[0], 1).copy()
        sent = np.full((e.num_anchors, e.head_channels), np.float32(7.5), np.float32)
        e.write_head(sent, 1)
        assert np.array_equal(e.read_tap(TAPS[0], 1), first)
        assert np.array_equal(e.debug_read_head_raw(1), sent)
