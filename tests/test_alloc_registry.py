"""Every device allocation of an engine goes through dev_alloc, and dev_alloc does not compile without a name and a class
(tests/test_gpu_mem_residue.py fills device memory by that registry: a range outside it would be a range no test chooses the
residue of)."""
import glob
import os
import re
import subprocess

from conftest import ROOT
from irmv_detection_amd import _build

CSRC = os.path.join(ROOT, "irmv_detection_amd", "csrc")
# hipMalloc outside dev_alloc, by name:
#   engine.cpp pnp_reserve          the PnP solver object (irmv_pnp_*): no engine, five buffers written and read within one call
#   comm.cpp                        the RCCL weight broadcast of the multi-GPU path: no engine either
#   engine_hooks.cpp debug_lds_run  the LDS fill / probe's result buffer: no engine, allocated and freed within the call
EXEMPT = {("engine.cpp", "pnp_reserve"), ("comm.cpp", None), ("engine_hooks.cpp", "debug_lds_run")}


def _function_at(text, pos):
    """Name of the function whose body holds text[pos]: the last `name(...)` header at column 0 in front of it."""
    heads = list(re.finditer(r"^(?:[\w:<>\*&\s\"]+?)\b([\w:]+)\s*\([^;{]*\)\s*\{", text[:pos], re.M))
    return heads[-1].group(1) if heads else None


def test_every_hipmalloc_is_dev_alloc():
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        name = os.path.basename(path)
        if not name.endswith((".cpp", ".hip", ".hpp", ".h")):
            continue
        text = open(path).read()
        for m in re.finditer(r"\bhipMalloc\s*\(", text):
            fn = _function_at(text, m.start())
            if (name, None) in EXEMPT or (name, fn) in EXEMPT:
                continue
            found.append((name, fn))
    assert found == [("engine_graph.cpp", "irmv::dev_alloc")], found


def test_every_dev_alloc_call_names_and_classifies_its_range():
    calls = 0
    for path in sorted(glob.glob(os.path.join(CSRC, "engine*.cpp"))):
        for line in open(path):
            if "dev_alloc(e," in line and "int irmv::dev_alloc" not in line:
                calls += 1
                assert re.search(r"mem_(const|act|scratch|scratch_index|carried_index)\(", line), (os.path.basename(path), line.strip())
    assert calls >= 40


def test_an_unclassified_allocation_does_not_compile(tmp_path):
    body = '#include "engine_internal.hpp"\nint f(irmv_engine *e, void **p) { return irmv::dev_alloc(e, p, 16%s); }\n'
    flags = ["-std=c++17", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
    rcs = []
    for i, tail in enumerate(("", ', "x"', ', "x", mem_scratch(MEM_F32)')):
        src = tmp_path / f"a{i}.cpp"
        src.write_text(body % tail)
        rcs.append(subprocess.run([_build.hipcc()] + flags + [str(src)], capture_output=True).returncode)
    assert rcs[0] != 0 and rcs[1] != 0 and rcs[2] == 0, rcs
