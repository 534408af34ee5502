"""Plate patches on the GPU (include/irmv_hip.h, "plate patches"; csrc/k_patch.hip): irmv_engine_patches_at and the step's side
records against irmv_detection_amd.patches, the host reference that follows the kernel operation for operation -- bytes of the
patch and every field.

Smallest shapes: 128 x 96 source, 64 x 64 net, seeded weights, nk = 8.  The reference is always fed the frame the step saw
(irmv_engine_rotated_image; turned back for an engine with rotate180 = 0, whose frame is the buffer itself) and the float32
keypoints the kernel saw.  tests/test_patches.py asserts, on the CPU, that the seeded quads keep their distance from every
rounding edge and that the step frames have survivors.
"""
import ctypes as C

import numpy as np
import pytest

import patch_set as PS
from irmv_detection_amd import capi, patches as PT
from irmv_detection_amd.engine import YoloEngine

pytestmark = pytest.mark.gpu

SRC, NET = PS.SRC, PS.NET
WIN = (64, 64)
ZERO = bytes(capi.PlatePatch())


def eng(blob, src=SRC, **kw):
    return YoloEngine(None, src, weights_blob=blob, net_size=NET[0], net_height=NET[1], score_thr=PS.STEP_THR, **kw)


def put(e, img, rot, slot=0):
    e.get_src_image_buffer(slot)[:] = PS.to_buffer(img, rot)


def seen(e, slot, rot):
    """The frame the slot's step saw, in the coordinates its results come in."""
    img = e.get_rotated_image(slot)
    return img if rot else np.ascontiguousarray(img[::-1, ::-1])


def check_slot(e, slot, rot, local=None, opts=None):
    """Every record of the slot against the reference on the frame its step saw.  local: the window-local float32 keypoints
    [n, 8] where the results' are shifted by a corner.  -> (records, records with state 1)."""
    img = seen(e, slot, rot)
    dets, ps = e.results_raw(slot), e.plate_patches(slot)
    assert len(ps) == len(dets)
    solved = 0
    for i, (d, p) in enumerate(zip(dets, ps)):
        if d.armor_valid != 1:
            assert bytes(p) == ZERO, (slot, i)
            continue
        k = np.array(list(d.kpts), np.float32) if local is None else local[i]
        want = PT.patch(img, k, d.armor_size, opts)
        got = PS.fields(p)
        assert PS.same(got, want), (slot, i, {f: (got[f], want[f]) for f in ("state", "otsu", "n_outside", "sum", "bar_sum")},
                                    int((got["gray"] != want["gray"]).sum()))
        assert bytes(p)[588:] == b"\0\0\0\0"
        solved += want["state"]
    return len(dets), solved


# ---- 1. patches_at ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(blob):
    with eng(blob) as e:
        put(e, PS.frame(0), True)
        e.detect()
        yield e


def test_patches_at_on_the_seeded_set(plain, capsys):
    """n = 1, 5, 64, 100, 256: a partial workgroup, every wave index, several workgroups; and n = 0.  The engine has never
    been enabled: the call stands on its own."""
    k, s = PS.quad_set()
    ref = PS.quad_set_reference()
    assert plain.patches_at(k[:0], s[:0]) == []
    start = checked = 0
    for n in (1, 5, 64, 100, 256):
        idx = (start + np.arange(n)) % len(k)
        start += n
        out = plain.patches_at(k[idx], s[idx])
        assert len(out) == n
        for j, i in enumerate(idx):
            got = PS.fields(out[j])
            assert PS.same(got, ref[i]), (n, j, int(i), int((got["gray"] != ref[i]["gray"]).sum()), got["otsu"], ref[i]["otsu"])
            checked += 1
    assert checked == 426 and start > len(k)      # (every quad of the set was asked at least once)
    with capsys.disabled():
        print(f"\n[patches] patches_at: {checked} records equal the reference's bytes")
    with pytest.raises(capi.IrmvError):
        plain.patches_at(np.zeros((257, 8), np.float32), 0)
    with pytest.raises(capi.IrmvError):
        plain.patches_at(k[:2], [0, 2])


def test_patches_at_on_hard_quads(plain):
    cases = PS.hard_quads()
    opts_now = None
    try:
        for name, k, size, opts, fr, state in cases:
            if opts != opts_now:      # the call runs under the engine's present options: set without enabling
                o = PT.options(opts)
                plain.set_patches(False, o["span"], o["light_rows"], o["top"])
                opts_now = opts
            put(plain, PS.hard_frame(fr), True)
            got = PS.fields(plain.patches_at(k[None], size)[0])
            want = PT.patch(PS.hard_frame(fr), k, size, opts)
            assert PS.same(got, want), (name, {f: (got[f], want[f]) for f in ("state", "otsu", "n_outside", "sum", "bar_sum")})
            if state is not None:
                assert got["state"] == state, name
    finally:
        plain.set_patches(False)
        put(plain, PS.frame(0), True)
        plain.detect()


# ---- 2. in the step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [True, False], ids=["rotate180", "unrotated"])
def test_single_and_batched_steps(blob, rot, capsys):
    with eng(blob, rotate180=rot, num_slots=3) as e:
        e.set_patches()
        assert e.patches() == dict(enable=True, span=(32, 54), light_rows=12, top=7)
        put(e, PS.step_frame(0), rot)
        e.detect()
        n, solved = check_slot(e, 0, rot)
        assert PS.STEP_MIN <= n <= PS.STEP_MAX_DET and solved >= PS.STEP_MIN
        for s in range(3):
            put(e, PS.step_frame(2 - s), rot, s)
        e.submit(0, 3)
        e.wait_slots(0, 3)
        counts = [check_slot(e, s, rot) for s in range(3)]
        assert all(c[1] >= PS.STEP_MIN for c in counts)
        assert len({bytes(e.plate_patches(s)[0]) for s in range(3)}) == 3      # three frames, three first patches
    with capsys.disabled():
        print(f"\n[patches] step, rotate180 = {rot}: single {(n, solved)}, batched {counts}")


def _local_kpts(p, crop, n):
    """The window-local keypoints of a window step: those of the plain engine of the window's size on the window's pixels
    (tests/test_gpu_window.py: the two are the same bits) -- result keypoints are these plus the corner, rounded to float32,
    which subtracting the corner does not undo."""
    put(p, crop, True)
    p.detect()
    d = p.results_raw(0)
    assert len(d) == n
    return [np.array(list(x.kpts), np.float32) for x in d]


def test_window_engine_moves_and_frame_view(blob, capsys):
    img = PS.step_frame(1)
    seen_n = []
    with eng(blob, window=WIN) as e, eng(blob, src=WIN) as p:
        e.set_patches()
        put(e, img, True)
        for view, org in (("window", (0, 0)), ("window", (37, 22)), ("window", (64, 32)), ("frame", (0, 0)), ("window", (11, 5))):
            e.set_view(view)
            if view == "window":
                e.set_window(*org)
            e.detect()
            dets = e.results_raw(0)
            local = None
            if view == "window":
                local = _local_kpts(p, img[org[1]:org[1] + WIN[1], org[0]:org[0] + WIN[0]], len(dets))
                o = np.tile(np.array(org, np.float32), 4)
                assert all(np.array_equal(np.array(list(d.kpts), np.float32), l + o) for d, l in zip(dets, local))
            assert e.get_rotated_image(0).shape[:2] == ((WIN[1], WIN[0]) if view == "window" else (SRC[1], SRC[0]))
            seen_n.append(check_slot(e, 0, True, local))
    with capsys.disabled():
        print(f"\n[patches] window engine: {seen_n}")
    assert all(s[1] >= 1 for s in seen_n) and sum(s[1] for s in seen_n) >= PS.STEP_MIN


def test_bayer_engine(blob):
    raw = PS.frame(5)[..., 1]
    with eng(blob, src_format="GRBG") as e:
        e.set_patches()
        e.get_src_image_buffer(0)[:] = raw
        e.detect()
        n, solved = check_slot(e, 0, True)
        assert solved >= 1


@pytest.mark.parametrize("source", [capi.POINTS_CLASSICAL, capi.POINTS_REFINED], ids=["classical", "refined"])
def test_classical_and_refined_engines(blob, source):
    """Behind the light extraction: a classical engine's records without an armor are all zero, a refined engine's patches are
    those of the points it finally reports."""
    with eng(blob, point_source=source) as e:
        e.set_patches()
        put(e, PS.step_frame(0), True)
        e.detect()
        n, solved = check_slot(e, 0, True)
        assert n >= PS.STEP_MIN
        valid = sum(d.armor_valid == 1 for d in e.results_raw(0))
        if source == capi.POINTS_CLASSICAL:
            assert sum(bytes(p) == ZERO for p in e.plate_patches(0)) >= n - valid
        else:
            assert solved >= 1


def test_run_post_on_an_injected_head(blob):
    """The head of another frame's step, injected: the records are that head's, the pixels the slot's present frame's."""
    with eng(blob) as e:
        e.set_patches()
        put(e, PS.step_frame(2), True)
        e.detect()
        head = e.read_head(0)
        kp = [bytes(d) for d in e.results_raw(0)]
        put(e, PS.step_frame(0), True)
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] != kp
        e.write_head(head, 0)
        e.run_post(0, 1)
        assert [bytes(d) for d in e.results_raw(0)] == kp
        n, solved = check_slot(e, 0, True)
        assert solved >= PS.STEP_MIN


def test_tiled_step_records_by_tile_and_index(blob):
    img = PS.step_frame(1)
    corners = [(0, 0), (40, 20)]
    with eng(blob, window=WIN, num_slots=3) as e, eng(blob, src=WIN) as p:
        e.set_patches()
        for s in range(3):
            put(e, img, True, s)
        e.set_tiles(corners, 1)
        e.submit_tiles(0, 1, 2)
        e.wait_slots(1, 2)
        recs, _ = e.tile_results_raw(1)
        ps = [e.plate_patches(1 + t) for t in range(2)]
        dets = [e.results_raw(1 + t) for t in range(2)]
        local = [_local_kpts(p, img[y:y + WIN[1], x:x + WIN[0]], len(dets[t])) for t, (x, y) in enumerate(corners)]
        solved = sum(check_slot(e, 1 + t, True, local[t])[1] for t in range(2))
        assert solved >= 1 and len(recs) >= 1
        for r in recs:                      # the patch of merged record r
            assert bytes(r.det) == bytes(dets[r.tile][r.index])
            want = PT.patch(img[corners[r.tile][1]:corners[r.tile][1] + WIN[1], corners[r.tile][0]:corners[r.tile][0] + WIN[0]],
                            local[r.tile][r.index], r.det.armor_size)
            assert PS.same(PS.fields(ps[r.tile][r.index]), want)


# ---- 3. liveness -------------------------------------------------------------------------------------------------------------
def test_liveness(blob):
    img = PS.step_frame(0)
    with eng(blob) as never, eng(blob) as e:
        for x in (never, e):
            put(x, img, True)
        never.detect()
        want = [bytes(d) for d in never.results_raw(0)]
        assert len(want) >= PS.STEP_MIN
        n = C.c_int(0)
        assert e._L.irmv_engine_plate_patches(e._h, 0, (capi.PlatePatch * e.max_det)(), e.max_det, C.byref(n)) == capi.ERR_ARG
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] == want
        e.set_patches()
        e.detect()
        g0 = e.debug_graph_count()
        assert [bytes(d) for d in e.results_raw(0)] == want
        assert check_slot(e, 0, True)[1] >= PS.STEP_MIN
        e.set_patches(span=(40, 60))
        e.detect()
        assert check_slot(e, 0, True, opts=dict(span=(40, 60)))[1] >= PS.STEP_MIN
        e.set_patches(enable=False)
        assert len(e.plate_patches(0)) == len(want) and all(bytes(p) == ZERO for p in e.plate_patches(0))
        e.detect()
        assert [bytes(d) for d in e.results_raw(0)] == want
        assert all(bytes(p) == ZERO for p in e.plate_patches(0))
        e.set_patches()
        assert all(bytes(p) == ZERO for p in e.plate_patches(0))          # nothing of the last enabled step is shown
        e.detect()
        assert check_slot(e, 0, True)[1] >= PS.STEP_MIN
        assert e.debug_graph_count() == g0
        with pytest.raises(capi.IrmvError):
            e.set_patches(span=(33, 54))
        assert e.patches()["span"] == (32, 54)


# ---- 4. memory residue -----------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_what_device_memory_held(blob):
    """The comparison of tests/mem_residue.py for the patch records: filled device memory against a fresh engine."""
    k, s = PS.quad_set()

    def go(fill):
        with eng(blob) as e:
            e.set_patches()
            put(e, PS.step_frame(0), True)
            e.detect()
            at0 = [bytes(p) for p in e.patches_at(k[:7], s[:7])]
            names = {r["name"]: r["cls"] for r in e.debug_allocs()}
            assert names["patch_dev"] == "SCRATCH" and names["patch_table"] == "CONST"
            assert all(names[n] == "SCRATCH" for n in ("patch_at_kpts", "patch_at_sizes", "patch_at_out"))
            if fill is not None:
                assert e.debug_fill_mem(fill) > 0
            e.detect()
            return [bytes(d) for d in e.results_raw(0)], [bytes(p) for p in e.plate_patches(0)], [bytes(p) for p in e.patches_at(k[:7], s[:7])], at0

    fresh = go(None)
    assert sum(capi.PlatePatch.from_buffer_copy(b).state == 1 for b in fresh[1]) >= PS.STEP_MIN and fresh[2] == fresh[3]
    for pattern in (0xFFFFFFFF, 0x7C007C00):
        assert go(pattern) == fresh
