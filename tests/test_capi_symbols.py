"""The C-ABI library loads on a CPU-only host, exports every symbol the header
declares, its structs agree with the ctypes mirror, and it refuses to compute
without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from irmv_detection_amd import _build, capi

HEADER = os.path.join(ROOT, "include", "irmv_hip.h")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(irmv_[a-z0-9_]+)\s*\(", text))
    assert len(declared) >= 30
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert declared == bound, declared ^ bound
    for name in declared:
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu'
                   ' %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(irmv_engine_cfg), sizeof(irmv_det), sizeof(irmv_raw_dets), sizeof(irmv_kernel_stat),'
                   'offsetof(irmv_engine_cfg, camera_matrix), offsetof(irmv_engine_cfg, weights_path), offsetof(irmv_det, rvec),'
                   'sizeof(irmv_conv_seg), sizeof(irmv_conv_op), sizeof(irmv_conv_cand), offsetof(irmv_conv_op, res),'
                   'offsetof(irmv_conv_op, fuse_layer), offsetof(irmv_conv_op, kname_one), offsetof(irmv_conv_cand, forced));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    exp = [C.sizeof(capi.EngineCfg), C.sizeof(capi.Det), C.sizeof(capi.RawDets), C.sizeof(capi.KernelStat),
           capi.EngineCfg.camera_matrix.offset, capi.EngineCfg.weights_path.offset, capi.Det.rvec.offset,
           C.sizeof(capi.ConvSeg), C.sizeof(capi.ConvOp), C.sizeof(capi.ConvCand), capi.ConvOp.res.offset,
           capi.ConvOp.fuse_layer.offset, capi.ConvOp.kname_one.offset, capi.ConvCand.forced.offset]
    assert got == exp


def test_graph_op_record_matches_the_header(tmp_path):
    """irmv_graph_op (irmv_engine_ops) against its ctypes mirror, field by field."""
    fields = [f for f, _ in capi.GraphOp._fields_]
    src = tmp_path / "go.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu", sizeof(irmv_graph_op));' +
                   "".join(f'printf(" %zu", offsetof(irmv_graph_op, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "go"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.GraphOp)] + [getattr(capi.GraphOp, f).offset for f in fields]


def test_op_io_record_matches_the_header(tmp_path):
    """irmv_op_io (irmv_engine_op_io) against its ctypes mirror, field by field."""
    fields = [f for f, _ in capi.OpIo._fields_]
    src = tmp_path / "io.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu", sizeof(irmv_op_io));' +
                   "".join(f'printf(" %zu", offsetof(irmv_op_io, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "io"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.OpIo)] + [getattr(capi.OpIo, f).offset for f in fields]


def test_light_trace_record_matches_the_header(tmp_path, lib):
    """irmv_light_trace / irmv_light_rec (irmv_engine_light_trace) against their ctypes mirrors, field by field, and the
    limits the library was compiled with against the header's array bounds."""
    parts = ['printf("%zu %zu", sizeof(irmv_light_trace), sizeof(irmv_light_rec));']
    parts += [f'printf(" %zu", offsetof(irmv_light_trace, {f}));' for f, _ in capi.LightTrace._fields_]
    parts += [f'printf(" %zu", offsetof(irmv_light_rec, {f}));' for f, _ in capi.LightRec._fields_]
    src = tmp_path / "lt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(parts) + "return 0;}\n")
    exe = tmp_path / "lt"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(capi.LightTrace), C.sizeof(capi.LightRec)] + [getattr(capi.LightTrace, f).offset for f, _ in capi.LightTrace._fields_] +
                   [getattr(capi.LightRec, f).offset for f, _ in capi.LightRec._fields_])
    L = capi.light_limits()
    assert (L["max_contours"], L["points_cap"]) == (capi.LIGHT_MAX_CONTOURS, capi.LIGHT_POINTS_CAP)
    assert L["lds_image"] > 0 and L["lds_points"] > 0


def test_sppf_slab_rule(lib):
    """The SPPF launch's slab rule (host only, no GPU needed): the widest slab whose four [H*W][CW] fp16 images fit in
    150 KiB of LDS and that still gives >= 768 workgroups, else the narrowest that fits; 0 = the global-memory kernel."""
    P5 = 128                                                   # model.9.m: 128 channels per slice
    assert lib.irmv_sppf_slab(1, 20, 20, P5) == 8             # 640 net, one frame
    assert lib.irmv_sppf_slab(1, 2, 2, P5) == 8               # 64 net
    assert lib.irmv_sppf_slab(192, 2, 2, P5) == 32            # 192 * 128 / 32 = 768 workgroups
    assert lib.irmv_sppf_slab(191, 2, 2, P5) == 16
    assert lib.irmv_sppf_slab(96, 2, 2, P5) == 16             # 96 * 128 / 16 = 768
    assert lib.irmv_sppf_slab(95, 2, 2, P5) == 8
    assert lib.irmv_sppf_slab(1, 48, 48, P5) == 8             # 1536 net: 4 * 2304 * 8 * 2 = 147456 B fit
    assert lib.irmv_sppf_slab(1, 49, 49, P5) == 0             # 1568 net: 153664 B > 150 KiB
    assert lib.irmv_sppf_slab(1, 64, 64, P5) == 0             # 2048 net
    assert lib.irmv_sppf_slab(1, 38, 64, P5) == 0             # 2048 x 1216: 2432 pixels
    assert lib.irmv_sppf_slab(1, 64, 2, P5) == 8 and lib.irmv_sppf_slab(1, 2, 64, P5) == 8
    assert lib.irmv_sppf_slab(0, 2, 2, P5) == capi.ERR_ARG and lib.irmv_sppf_slab(1, 2, 2, 12) == capi.ERR_ARG


def test_defaults_are_the_reference_constants(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    assert (cfg.src_width, cfg.src_height, cfg.net_size) == (1280, 1024, 640)
    assert cfg.rotate180 == 1 and cfg.swap_rb == 0 and cfg.resize_mode == capi.RESIZE_STRETCH
    assert cfg.num_slots == 3 and cfg.max_det == 100 and cfg.armor_size == capi.ARMOR_SMALL
    assert abs(cfg.camera_matrix[0] - 957.669211) < 1e-12 and abs(cfg.dist_coeffs[0] + 0.405274) < 1e-12   # config/camera_info.yaml
    assert lib.irmv_version().startswith(b"irmv_hip")


def test_bad_arguments_are_rejected_before_touching_the_gpu(lib):
    cfg = capi.EngineCfg()
    lib.irmv_engine_cfg_default(C.byref(cfg))
    h = C.c_void_p()
    cfg.net_size = 100
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
    assert b"net_size" in lib.irmv_last_error()
    cfg.net_size = 640
    cfg.struct_size = 4
    assert lib.irmv_engine_create(C.byref(cfg), C.byref(h)) == capi.ERR_ARG
    assert lib.irmv_engine_create(None, C.byref(h)) == capi.ERR_ARG
    assert lib.irmv_engine_src_buffer(None, 0) is None or not lib.irmv_engine_src_buffer(None, 0)


def test_no_cpu_fallback(lib, blob):
    """Without a HIP device the product path must fail loudly."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from irmv_detection_amd.engine import PnPSolver, YoloEngine
    with pytest.raises(capi.IrmvError) as ei:
        YoloEngine(None, (1280, 1024), weights_blob=blob)
    assert ei.value.code == capi.ERR_HIP
    with pytest.raises(capi.IrmvError):
        PnPSolver([1, 0, 0, 0, 1, 0, 0, 0, 1], [0] * 5)


def test_numa_cpulist_parser_and_thread_binding(lib):
    """Host-side NUMA placement (csrc/numa.hpp): the sysfs cpulist parser, and binding a thread to a node's CPUs within the
    process's own cpuset.  Runs in a child process: affinity is per thread, and the test runner's must stay as it is."""
    assert capi.numa_parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    assert capi.numa_parse_cpulist("5") == [5]
    assert capi.numa_parse_cpulist("") == [] and capi.numa_parse_cpulist("\n") == []
    assert capi.numa_parse_cpulist("0-1, 4-5") == [0, 1, 4, 5]
    assert capi.numa_parse_cpulist("3-1") == []                    # malformed range: nothing is bound rather than something wrong
    assert capi.numa_parse_cpulist("0-2,x,7") == [0, 1, 2]         # parsing stops at the first thing it does not understand
    assert len(capi.numa_parse_cpulist("0-127")) == 128
    node0 = "/sys/devices/system/node/node0/cpulist"
    if not os.path.exists(node0):
        pytest.skip("no NUMA topology in sysfs")
    code = ("import os, sys; sys.path.insert(0, %r)\n"
            "from irmv_detection_amd import capi\n"
            "L = capi.load()\n"
            "before = os.sched_getaffinity(0)\n"
            "want = set(capi.numa_parse_cpulist(open(%r).read())) & before\n"
            "rc = L.irmv_numa_bind_thread(0)\n"
            "after = os.sched_getaffinity(0)\n"
            "assert (rc == 0 and after == want) or (rc != 0 and after == before and not want), (rc, before, after, want)\n"
            "assert L.irmv_numa_bind_thread(4095) != 0 and os.sched_getaffinity(0) == after\n"   # no such node: refused, nothing changed
            "buf = bytearray(8192); import ctypes as C\n"
            "n = L.irmv_numa_page_node(C.addressof(C.c_char.from_buffer(buf)))\n"
            "assert n >= -1\n"
            "print('ok', rc, sorted(after)[:4], n)\n") % (ROOT, node0)
    out = subprocess.check_output([os.sys.executable, "-c", code], text=True)
    assert out.startswith("ok")


def test_mem_range_record_matches_the_header(tmp_path):
    """irmv_mem_range (irmv_engine_debug_allocs) against its ctypes mirror, field by field, and the class / kind numbers."""
    fields = [f for f, _ in capi.MemRange._fields_]
    src = tmp_path / "mr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu", sizeof(irmv_mem_range));' +
                   "".join(f'printf(" %zu", offsetof(irmv_mem_range, {f}));' for f in fields) +
                   'printf(" %d %d %d %d %d %d %d %d %d", IRMV_MEM_CONST, IRMV_MEM_ACT, IRMV_MEM_CARRIED, IRMV_MEM_SCRATCH,'
                   ' IRMV_MEM_U8, IRMV_MEM_F16, IRMV_MEM_F32, IRMV_MEM_F64, IRMV_MEM_INDEX);return 0;}\n')
    exe = tmp_path / "mr"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(capi.MemRange)] + [getattr(capi.MemRange, f).offset for f in fields] +
                   [capi.MEM_CLASSES.index(c) for c in ("CONST", "ACT", "CARRIED", "SCRATCH")] +
                   [capi.MEM_KINDS.index(k) for k in ("U8", "F16", "F32", "F64", "INDEX")])
