"""Plate numbers on the GPU (include/irmv_hip.h, "plate numbers"; csrc/k_number.hip): irmv_engine_numbers_at and the step's
side records against irmv_detection_amd.number_net.NumberModel.reference, the host reference that follows the kernel operation
for operation -- bytes of whole 96-byte records, never a tolerance.  tests/test_number_net.py holds that reference to an
independent restatement on the CPU.

Smallest shapes: those of tests/patch_set.py (128 x 96 source, 64 x 64 net, seeded weights).  numbers_at needs no frame: its
patches are the host patch reference's on the seeded quad set.  The models are seeded; their widths are the ones at which the
kernel takes another path: one unit a lane and two (64 | 65), the padding of 16 (1, 63, 65, 127), C = 1 (no runner-up), 2, 16.
Every step form is checked against reference(plate_patches(slot)) and must show a record with state 1.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import patch_set as PS
import test_gpu_patches as TP
import test_gpu_side_records as SR
from irmv_detection_amd import capi, number_net as NN

pytestmark = pytest.mark.gpu

ZERO = bytes(capi.PlateNumber())
MAIN = [560, 64, 9]
SHAPES = ([560, 9], MAIN, [560, 128, 100, 16],
          [560, 1], [560, 2], [560, 16], [560, 1, 2], [560, 63, 16], [560, 65, 1], [560, 127, 65, 2], [560, 64, 127, 16], [560, 128, 1, 9])


@functools.lru_cache(maxsize=None)
def model(dims=tuple(MAIN), seed=0, input="binary"):
    r = np.random.RandomState(500 + seed + sum(dims))
    ws = [(r.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [(r.standard_normal(dims[l + 1]) * 0.3).astype(np.float32) for l in range(len(dims) - 1)]
    return NN.NumberModel(ws, bs, input)


def patch_struct(p: dict) -> capi.PlatePatch:
    """A patches.patch dict as the record the kernel reads."""
    s = capi.PlatePatch()
    C.memmove(C.byref(s), np.ascontiguousarray(p["gray"], np.uint8).tobytes(), 560)
    s.state, s.otsu, s.n_outside, s.armor_size, s.sum = p["state"], p["otsu"], p["n_outside"], p["armor_size"], p["sum"]
    s.bar_sum[0], s.bar_sum[1] = p["bar_sum"]
    return s


@functools.lru_cache(maxsize=None)
def seeded():
    """The quad set's patches on frame 0 (tests/patch_set.py, computed once) as records."""
    return tuple(patch_struct(p) for p in PS.quad_set_reference())


@functools.lru_cache(maxsize=None)
def seeded_reference(dims, input):
    out = model(dims, 0, input).reference(list(seeded()))
    out.setflags(write=False)
    return out


def crafted(gray, otsu, state=1):
    g = np.broadcast_to(np.asarray(gray, np.uint8), (560,)) if np.ndim(gray) < 2 else np.asarray(gray, np.uint8).reshape(560)
    return patch_struct(dict(gray=g, state=state, otsu=otsu, n_outside=0, armor_size=0, sum=int(g.astype(np.int64).sum()), bar_sum=(0, 0)))


def same(got, want):
    return NN.records(got).tobytes() == np.asarray(want, NN.NUMBER_DTYPE).tobytes()


def check_slot(e, slot, m):
    """The slot's number records against the reference on the slot's own patch records -> (records, records with state 1)."""
    ps, ns = e.plate_patches(slot), e.plate_numbers(slot)
    assert len(ns) == len(ps) == len(e.results_raw(slot))
    want = m.reference(ps)
    got = NN.records(ns)
    assert got.tobytes() == want.tobytes(), (slot, [i for i in range(len(ns)) if got[i].tobytes() != want[i].tobytes()][:5])
    assert [n.state for n in ns] == [p.state for p in ps]
    return len(ns), int(sum(n.state == 1 for n in ns))


def numbered(e, m=None):
    e.set_number_model(m or model())
    e.set_numbers()
    return e


# ---- 1. numbers_at -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(blob):
    with TP.eng(blob) as e:
        yield e


@pytest.mark.parametrize("input", ["binary", "gray"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_numbers_at_on_the_seeded_patches(plain, dims, input):
    """n = 1, 5, 64, 100, 256: a partial workgroup, every wave index, several workgroups; and n = 0.  The op has never been
    enabled on this engine: the call stands on its own."""
    src, ref = seeded(), seeded_reference(tuple(dims), input)
    assert sum(p.state == 1 for p in src) >= 390
    plain.set_number_model(model(tuple(dims), 0, input))
    assert plain.numbers_at([]) == []
    start = 0
    for n in (1, 5, 64, 100, 256):
        idx = (start + np.arange(n)) % len(src)
        start += n
        out = plain.numbers_at([src[i] for i in idx])
        assert len(out) == n
        got = NN.records(out)
        bad = [int(i) for j, i in enumerate(idx) if got[j].tobytes() != ref[i].tobytes()]
        assert not bad, (n, bad[:5], got[0] if n == 1 else None, ref[idx[0]])
    assert start > len(src)          # (every patch of the set was asked at least once)
    with pytest.raises(capi.IrmvError):
        plain.numbers_at([src[0]] * 257)


@pytest.mark.parametrize("input", ["binary", "gray"])
def test_numbers_at_on_crafted_patches(plain, input):
    r = np.random.RandomState(3)
    noise = r.randint(0, 256, 560).astype(np.uint8)
    for dims in ((560, 9), tuple(MAIN), (560, 128, 100, 16)):
        m = model(dims, 1, input)
        plain.set_number_model(m)
        cases = [crafted(0, 0, state=0), capi.PlatePatch(),                      # "no answer"
                 crafted(93, 93), crafted(0, 0), crafted(255, 255),              # one level: binary mode sees no one at all
                 crafted(255, 0), crafted(255, 254),                             # all 255: every input one
                 crafted(noise, 0), crafted(noise, 255), crafted(noise, 128),    # otsu at both ends
                 crafted(np.arange(560) % 256, 127)]
        out = plain.numbers_at(cases)
        want = m.reference(cases)
        assert same(out, want), [i for i in range(len(cases)) if bytes(out[i]) != want[i].tobytes()]
        assert bytes(out[0]) == ZERO and bytes(out[1]) == ZERO and all(o.state == 1 for o in out[2:])
        if input == "binary":
            # all x are 0: the logits are the biases pushed through the layers
            a = m.biases[0][None]
            for l in range(1, m.n_layers):
                a = NN.NumberModel._layer(np.where(a > 0, a, np.float32(0)).astype(np.float32), m.w16[l], m.biases[l])
            a = a[0]
            for k in (2, 3, 4):
                assert out[k].ones == 0 and np.array_equal(np.array(list(out[k].logits), np.float32)[:dims[-1]], a)
            assert out[5].ones == 560 and out[6].ones == 560 and out[8].ones == 0
            assert out[7].ones == int((noise > 0).sum())
        else:
            assert out[5].ones == 560 * 255 and out[2].ones == 560 * 93 and out[7].ones == out[8].ones == int(noise.astype(np.int64).sum())
    for state, otsu in ((2, 10), (-1, 10), (1, -1), (1, 256), (0, 256)):
        with pytest.raises(capi.IrmvError) as ei:
            plain.numbers_at([crafted(noise, 10), crafted(noise, otsu, state=state)])
        assert ei.value.code == capi.ERR_ARG


def test_numbers_at_ties(plain):
    """Identical weight rows: the smaller index is the label, the other the runner-up, margin 0 -- through one layer and two."""
    r = np.random.RandomState(8)
    w = (r.standard_normal((16, 560)) * 0.05).astype(np.float32)
    w[11] = w[3]
    w[[i for i in range(16) if i not in (3, 11)]] -= 1.0
    b = np.zeros(16, np.float32)
    w2 = (r.standard_normal((5, 16)) * 0.1).astype(np.float32)
    w2[4] = w2[2] = np.abs(w2[2]) + 1.0
    for m, pair in ((NN.NumberModel([w], [b]), (3, 11)), (NN.NumberModel([np.abs(w), w2], [b, np.zeros(5, np.float32)]), (2, 4)),
                    (NN.NumberModel([np.tile(w[3], (3, 1))], [b[:3]]), (0, 1))):
        plain.set_number_model(m)
        src = [seeded()[i] for i in range(40)]
        out = plain.numbers_at(src)
        assert same(out, m.reference(src))
        live = [o for o in out if o.state == 1]
        assert len(live) >= 30 and all((o.label, o.second, o.margin) == (pair[0], pair[1], 0.0) for o in live)


# ---- 2. in the step ----------------------------------------------------------------------------------------------------------
ZC = pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "device_records"])


def set_zero_copy(monkeypatch, zero_copy):
    if not zero_copy:
        monkeypatch.setenv("IRMV_ZERO_COPY_RESULTS", "0")


@ZC
def test_detect_batched_and_run_post(blob, zero_copy, monkeypatch, capsys):
    set_zero_copy(monkeypatch, zero_copy)
    m = model()
    with TP.eng(blob, num_slots=3) as e:
        numbered(e, m)
        assert e.numbers() == dict(enable=True) and e.patches()["enable"]
        TP.put(e, PS.step_frame(0), True)
        e.detect()
        one = check_slot(e, 0, m)
        TP.check_slot(e, 0, True)
        for s in range(3):
            TP.put(e, PS.step_frame(2 - s), True, s)
        e.submit(0, 3)
        e.wait_slots(0, 3)
        batched = [check_slot(e, s, m) for s in range(3)]
        assert len({bytes(e.plate_numbers(s)[0]) for s in range(3)}) == 3      # three frames, three first records
        # run_post on the head of slot 0's step (frame 2) while the slot holds frame 0
        head = e.read_head(0)
        of_head = [bytes(d) for d in e.results_raw(0)]
        TP.put(e, PS.step_frame(0), True)
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] != of_head
        e.write_head(head, 0)
        e.run_post(0, 1)
        assert [bytes(d) for d in e.results_raw(0)] == of_head
        post = check_slot(e, 0, m)
        TP.check_slot(e, 0, True)
    with capsys.disabled():
        print(f"\n[numbers] zero_copy = {zero_copy}: detect {one}, batched {batched}, run_post {post}")
    assert one[1] >= 1 and all(b[1] >= 1 for b in batched) and post[1] >= 1
    assert one[1] >= PS.STEP_MIN and sum(b[1] for b in batched) >= 3 * PS.STEP_MIN


@ZC
def test_window_engine_moves_frame_view_and_tiles(blob, zero_copy, monkeypatch, capsys):
    set_zero_copy(monkeypatch, zero_copy)
    m = model(tuple(MAIN), 0, "gray")
    img = PS.step_frame(1)
    seen = []
    with TP.eng(blob, window=TP.WIN, num_slots=3) as e:
        numbered(e, m)
        for s in range(3):
            TP.put(e, img, True, s)
        for view, org in (("window", (0, 0)), ("window", (37, 22)), ("frame", (0, 0)), ("window", (11, 5))):
            e.set_view(view)
            if view == "window":
                e.set_window(*org)
            e.detect()
            seen.append((view, check_slot(e, 0, m)))
        assert all(s[1][1] >= 1 for s in seen)
        # a tiled step: the number of merged record r is plate_numbers(first + r.tile)[r.index]
        e.set_tiles(SR.CORNERS, 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        tiles = [check_slot(e, 1 + t, m) for t in range(2)]
        recs, _ = e.tile_results_raw(1)
        ns = [e.plate_numbers(1 + t) for t in range(2)]
        ps = [e.plate_patches(1 + t) for t in range(2)]
        dets = [e.results_raw(1 + t) for t in range(2)]
        assert len(recs) >= 1
        live = 0
        for r in recs:
            assert bytes(r.det) == bytes(dets[r.tile][r.index])
            assert same([ns[r.tile][r.index]], m.reference([ps[r.tile][r.index]]))
            live += ns[r.tile][r.index].state
        assert live >= 1 and sum(t[1] for t in tiles) >= 1
    with capsys.disabled():
        print(f"\n[numbers] window engine, zero_copy = {zero_copy}: {seen}, tiled {tiles}, merged {len(recs)} ({live} classified)")


def test_bayer_engine(blob):
    m = model()
    with TP.eng(blob, src_format="GRBG") as e:
        numbered(e, m)
        e.get_src_image_buffer(0)[:] = PS.frame(5)[..., 1]
        e.detect()
        assert check_slot(e, 0, m)[1] >= 1
        TP.check_slot(e, 0, True)


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_classical_and_refined_engines(blob, source):
    """Behind the light extraction and the patch kernel behind it.  The classical engine sees the frame with two bars drawn in
    (tests/test_gpu_side_records.py): the seeded frames hold no light pair."""
    m = model()
    kw = dict(binary_threshold=250) if source == capi.POINTS_CLASSICAL else {}
    with TP.eng(blob, point_source=source, **kw) as e:
        numbered(e, m)
        TP.put(e, SR.barred(0) if source == capi.POINTS_CLASSICAL else PS.step_frame(0), True)
        e.detect()
        n, live = check_slot(e, 0, m)
        assert n >= 1 and live >= 1
        assert sum(bytes(r) == ZERO for r in e.plate_numbers(0)) == n - live


# ---- 3. liveness -------------------------------------------------------------------------------------------------------------
def test_liveness(blob):
    img = PS.step_frame(0)
    m, m2 = model(), model((560, 128, 100, 16), 2, "gray")
    with TP.eng(blob) as never, TP.eng(blob) as e:
        for x in (never, e):
            TP.put(x, img, True)
        never.detect()
        want = [bytes(d) for d in never.results_raw(0)]
        assert len(want) >= PS.STEP_MIN
        n = C.c_int(0)
        getter = lambda: e._L.irmv_engine_plate_numbers(e._h, 0, (capi.PlateNumber * e.max_det)(), e.max_det, C.byref(n))
        assert getter() == capi.ERR_ARG                       # before the first set
        e.set_numbers(False)                                  # switching off what was never on makes nothing
        assert getter() == capi.ERR_ARG and not [r for r in e.debug_allocs() if r["name"].startswith(("number", "patch"))]
        with pytest.raises(capi.IrmvError) as ei:             # enable without a model
            e.set_numbers()
        assert ei.value.code == capi.ERR_ARG and getter() == capi.ERR_ARG and not e.numbers()["enable"] and not e.patches()["enable"]
        with pytest.raises(capi.IrmvError):
            e.numbers_at([seeded()[0]])                       # ... and numbers_at needs one too
        assert not [r for r in e.debug_allocs() if r["name"].startswith("number")]
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] == want
        e.set_number_model(m)
        assert getter() == capi.ERR_ARG and same(e.numbers_at(list(seeded()[:5])), seeded_reference(tuple(MAIN), "binary")[:5])
        e.set_numbers()                                       # an engine without patches: they are turned on
        assert e.patches() == dict(enable=True, span=(32, 54), light_rows=12, top=7) and e.numbers()["enable"]
        e.detect()
        g0 = e.debug_graph_count()
        assert [bytes(d) for d in e.results_raw(0)] == want
        assert check_slot(e, 0, m)[1] >= PS.STEP_MIN and TP.check_slot(e, 0, True)[1] >= PS.STEP_MIN
        first = [bytes(r) for r in e.plate_numbers(0)]
        e.set_number_model(m2)                                # a model swap between two steps: live, no new capture
        assert [bytes(r) for r in e.plate_numbers(0)] == first
        e.detect()
        assert check_slot(e, 0, m2)[1] >= PS.STEP_MIN and [bytes(r) for r in e.plate_numbers(0)] != first
        assert e.debug_graph_count() == g0
        e.set_numbers(False)                                  # disable zeroes the records
        assert len(e.plate_numbers(0)) == len(want) and all(bytes(r) == ZERO for r in e.plate_numbers(0))
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] == want and all(bytes(r) == ZERO for r in e.plate_numbers(0))
        assert TP.check_slot(e, 0, True)[1] >= PS.STEP_MIN    # (the patches stay on)
        e.set_number_model(m)
        e.set_numbers()
        assert all(bytes(r) == ZERO for r in e.plate_numbers(0))          # nothing of the last enabled step is shown
        e.detect()
        assert check_slot(e, 0, m)[1] >= PS.STEP_MIN and [bytes(r) for r in e.plate_numbers(0)] == first
        e.set_patches(False)                                  # patches off, numbers on: every record is "no answer"
        e.detect()
        assert len(e.plate_numbers(0)) == len(want) and all(bytes(r) == ZERO for r in e.plate_numbers(0))
        assert e.numbers()["enable"]
        e.set_patches()
        e.detect()
        assert [bytes(r) for r in e.plate_numbers(0)] == first
        assert e.debug_graph_count() == g0
        with pytest.raises(capi.IrmvError):                   # a refused model changes nothing
            bad = NN.NumberModel(m.weights, m.biases)
            bad.weights[0] = bad.weights[0].copy(); bad.weights[0][0, 0] = np.inf
            e.set_number_model(bad)
        e.detect()
        assert [bytes(r) for r in e.plate_numbers(0)] == first


def test_model_from_an_irmn_file(blob, tmp_path):
    m = model((560, 63, 16), 0, "gray")
    path = str(tmp_path / "m.irmn")
    m.save(path)
    with TP.eng(blob) as e:
        e.set_number_model(path)
        src = list(seeded()[:9])
        assert same(e.numbers_at(src), m.reference(src))
        with pytest.raises(capi.IrmvError):
            e.set_number_model(str(tmp_path / "missing.irmn"))
        assert same(e.numbers_at(src), m.reference(src))


def test_an_engine_that_never_asks_has_nothing_of_it(blob):
    with TP.eng(blob) as e:
        e.set_patches()
        TP.put(e, PS.step_frame(0), True)
        e.detect()
        assert not [r for r in e.debug_allocs() if r["name"].startswith("number")]
        rows = [r["name"] for r in e.profile(0, 1)]
        assert "plate_patch" in rows and "plate_number" not in rows
        numbered(e)
        rows = [r["name"] for r in e.profile(0, 1)]
        assert rows.index("plate_number") == rows.index("plate_patch") + 1
        e.set_yaw_solve()                                     # (directly behind the NMS, in front of the two)
        rows = [r["name"] for r in e.profile(0, 1)]
        assert rows.index("plate_number") == rows.index("plate_patch") + 1 and "yaw_solve" in rows
        e.detect()
        assert check_slot(e, 0, model())[1] >= PS.STEP_MIN


# ---- 4. memory residue -----------------------------------------------------------------------------------------------------
@ZC
def test_records_do_not_depend_on_what_device_memory_held(blob, zero_copy, monkeypatch):
    """The comparison of tests/mem_residue.py for the number records: filled device memory against a fresh engine."""
    set_zero_copy(monkeypatch, zero_copy)
    src = list(seeded()[:7])

    def go(fill):
        with TP.eng(blob) as e:
            numbered(e)
            TP.put(e, PS.step_frame(0), True)
            e.detect()
            at0 = [bytes(r) for r in e.numbers_at(src)]
            names = {r["name"]: r["cls"] for r in e.debug_allocs()}
            assert names["number_dev"] == "SCRATCH" and all(names[n] == "CONST" for n in ("number_table", "number_weights", "number_bias"))
            assert all(names[n] == "SCRATCH" for n in ("number_at_in", "number_at_out"))
            if fill is not None:
                assert e.debug_fill_mem(fill) > 0
            e.detect()
            return [bytes(d) for d in e.results_raw(0)], [bytes(r) for r in e.plate_numbers(0)], [bytes(r) for r in e.numbers_at(src)], at0

    fresh = go(None)
    assert sum(capi.PlateNumber.from_buffer_copy(b).state == 1 for b in fresh[1]) >= PS.STEP_MIN and fresh[2] == fresh[3]
    for pattern in (0xFFFFFFFF, 0x7C007C00):
        assert go(pattern) == fresh


# ---- 5. all five side records together ---------------------------------------------------------------------------------------
FEATURES = SR.FEATURES + ("number",)
ENABLE = dict(SR.ENABLE, number=lambda e: numbered(e))
READ = dict(SR.READ, number=lambda e, s: [bytes(r) for r in e.plate_numbers(s)])
STEP_RECORDS = SR.STEP_RECORDS + ("number",)


@contextlib.contextmanager
def group(blob, **kw):
    """{name: engine}: all five features (in both orders) and one engine per feature.  The number engine turns its patches on
    itself; where `all` enables patches first, set_numbers finds them set."""
    plan = [("all", FEATURES), ("all_rev", FEATURES[::-1])] + [(f, (f,)) for f in FEATURES]
    with contextlib.ExitStack() as st:
        g = {}
        for name, feats in plan:
            g[name] = st.enter_context(TP.eng(blob, num_slots=SR.SLOTS, **kw))
            for f in feats:
                ENABLE[f](g[name])
        yield g


def compare(g, slots, form, live, seen):
    for s in slots:
        want = [bytes(d) for d in g["all"].results_raw(s)]
        for name, e in g.items():
            assert [bytes(d) for d in e.results_raw(s)] == want, (form, s, name)
    for f in FEATURES:
        one = [READ[f](g[f], s) for s in slots]
        for name in ("all", "all_rev"):
            assert [READ[f](g[name], s) for s in slots] == one, (form, f, name)
        seen[(form, f)] = sum(any(r) for recs in one for r in recs)
        if f in live:
            assert seen[(form, f)] >= 1, (form, f)
    # the number engine's own patches are the patch engine's
    assert [READ["patch"](g["number"], s) for s in slots] == [READ["patch"](g["patch"], s) for s in slots], form


@ZC
def test_all_five_side_records_on_one_engine(blob, zero_copy, monkeypatch, capsys):
    set_zero_copy(monkeypatch, zero_copy)
    seen = {}
    with group(blob) as g:
        a = g["all"]
        SR.each(g, lambda e: TP.put(e, PS.step_frame(0), True))
        SR.each(g, lambda e: e.detect())
        compare(g, [0], "detect", FEATURES, seen)
        check_slot(a, 0, model())
        for s in range(SR.SLOTS):
            SR.each(g, lambda e: TP.put(e, PS.step_frame(2 - s), True, s))
        SR.each(g, lambda e: e.submit(0, SR.SLOTS))
        SR.each(g, lambda e: e.wait_slots(0, SR.SLOTS))
        compare(g, range(SR.SLOTS), "submit", FEATURES, seen)
        heads = SR.each(g, lambda e: e.read_head(0))
        SR.each(g, lambda e: TP.put(e, PS.step_frame(0), True))
        SR.each(g, lambda e: e.detect())
        for e, h in zip(g.values(), heads):
            e.write_head(h, 0)
            e.run_post(0, 1)
        compare(g, [0], "run_post", STEP_RECORDS, seen)
        check_slot(a, 0, model())
    with group(blob, window=TP.WIN) as g:
        a = g["all"]
        for s in range(SR.SLOTS):
            SR.each(g, lambda e: TP.put(e, PS.step_frame(1), True, s))
        SR.each(g, lambda e: e.set_tiles(SR.CORNERS, 1))
        SR.each(g, lambda e: e.submit_tiles(0, 1, 2))
        SR.each(g, lambda e: e.wait_slots(1, 2))
        compare(g, [1, 2], "tiled", STEP_RECORDS, seen)
        SR.each(g, lambda e: e.set_view("frame"))
        SR.each(g, lambda e: e.detect())
        compare(g, [0], "frame view", FEATURES, seen)
        check_slot(a, 0, model())
    with capsys.disabled():
        print(f"\n[numbers] five side records, zero_copy = {zero_copy}: records not all zero {seen}")
