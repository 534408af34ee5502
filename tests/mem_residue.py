"""Helpers of tests/test_gpu_mem_residue.py: the engine's classified device ranges, the channels its ops declare as written,
and what the test computes from them itself -- the bytes a fill must cover, the pad channels that must stay +0, the carried
invariants."""
import ctypes as C

import numpy as np

from irmv_detection_amd import capi

PATTERNS = (0x00000000, 0x7e007e00, 0xfbfffbff, 0xffffffff)


def graph_ops(e):
    n = C.c_int(0)
    capi.check(e._L.irmv_engine_ops(e._h, None, 0, C.byref(n)))
    ops = (capi.GraphOp * n.value)()
    capi.check(e._L.irmv_engine_ops(e._h, ops, n.value, C.byref(n)))
    return list(ops)


def tensor_shape(e, name):
    shape = (C.c_int * 3)()
    capi.check(e._L.irmv_engine_read_tap(e._h, 0, name.encode(), None, shape))
    return tuple(shape)


def esize(name):
    return 4 if name.startswith("head.") else 2      # the head records are fp32, every other activation tensor fp16


def written_channels(e):
    """{tensor: sorted channels some op declares as written}: out_coff / out_C of irmv_engine_ops and the writes of
    irmv_engine_op_io (the fused ops; every other op answers IRMV_ERR_ARG)."""
    w = {}
    for o in graph_ops(e):
        if o.out_tensor:
            w.setdefault(o.out_tensor.decode(), set()).update(range(o.out_coff, o.out_coff + o.out_C))
        io = capi.OpIo()
        if e._L.irmv_engine_op_io(e._h, o.op, C.byref(io)) == capi.OK:
            for s in io.writes[:io.n_writes]:
                w.setdefault(s.tensor.decode(), set()).update(range(s.coff, s.coff + s.C))
    return {t: sorted(c) for t, c in w.items()}


def expected_fill_bytes(e, allocs=None):
    """The bytes fill_mem must cover, per class, from the registry and the op listings alone."""
    allocs = e.debug_allocs() if allocs is None else allocs
    scratch = sum(a["bytes"] for a in allocs if a["cls"] == "SCRATCH")
    act = 0
    for t, ch in written_channels(e).items():
        H, W, Ct = tensor_shape(e, t)
        assert ch and ch[-1] < Ct, (t, ch[-1], Ct)
        act += len(ch) * H * W * esize(t) * e.num_slots
    return dict(SCRATCH=scratch, ACT=act)


def read_tensor_bits(e, name, allocs=None):
    """The tensor's words on every slot as they lie in memory, read through the registry (no read-back step runs, no stale
    flag changes): uint16 / uint32 [slots, H, W, C].  A head level is its share of head_all: [level][slot][H * W][96]."""
    allocs = e.debug_allocs() if allocs is None else allocs
    H, W, Ct = tensor_shape(e, name)
    n = e.num_slots * H * W * Ct * esize(name)
    if name.startswith("head."):
        off = sum(e.num_slots * int(np.prod(tensor_shape(e, f"head.{l}"))) * 4 for l in range(int(name[5:])))
        idx = [i for i, a in enumerate(allocs) if a["name"] == "head_all"]
    else:
        off, idx = 0, [i for i, a in enumerate(allocs) if a["name"] == name and a["cls"] == "ACT"]
    assert len(idx) == 1 and allocs[idx[0]]["cls"] == "ACT", (name, idx)
    raw = e.debug_read_mem(idx[0], off, n)
    return raw.view(np.uint32 if esize(name) == 4 else np.uint16).reshape(e.num_slots, H, W, Ct)


def dirty_pad_channels(e, written=None):
    """[(tensor, channel)] of never-written channels that are not +0 bitwise on some slot."""
    written = written_channels(e) if written is None else written
    bad = []
    allocs = e.debug_allocs()
    for t, ch in written.items():
        bits = read_tensor_bits(e, t, allocs)
        pad = np.setdiff1d(np.arange(bits.shape[-1]), ch)
        if len(pad):
            nz = bits[..., pad].reshape(-1, len(pad)).any(axis=0)
            bad += [(t, int(c)) for c in pad[nz]]
    return bad


def carried_nonzero(e):
    """What of the two carried ranges is not zero: the candidate counters and the candidate-anchor bitmap of every slot."""
    bad = []
    counts = e.debug_cand_counts()
    if counts.any():
        bad.append(("cand_counts", counts.tolist()))
    for s in range(e.num_slots):
        _, words = e.debug_cand_bits(s)
        if words.any():
            bad.append(("cand_bits", s, int(np.count_nonzero(words))))
    return bad


def freeze(x):
    """Anything a read-back returns, as a hashable value that compares bit for bit."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(freeze(v) for v in x)
    if isinstance(x, (C.Structure, C.Array)):
        return bytes(x)
    return x
