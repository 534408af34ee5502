"""The debug images through the C++ facade and the detector core (tests/cpp/render_test.cpp): compiled here like the
programs of tests/test_cpp_facade.py (so the binary travels to the GPU box with the tree), run on the GPU."""
import os
import subprocess

import pytest

import detect_craft as dc
from conftest import ROOT
from irmv_detection_amd import _build

INC = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "_bin")
EXE = os.path.join(BIN, "render_test")


def _compile():
    os.makedirs(BIN, exist_ok=True)
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", INC, os.path.join(CPP, "render_test.cpp"), "-o", EXE,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


def test_render_program_compiles_against_the_facade():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_facade_and_core_render_on_gpu(tmp_path, blob):
    import numpy as np
    exe = EXE if os.path.exists(EXE) else _compile()
    crafted = dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))   # detections on every frame
    (tmp_path / "yolov7.irmw").write_bytes(crafted)
    np.random.default_rng(11).integers(0, 256, (68, 100, 3), dtype=np.uint8).tofile(tmp_path / "frame.bin")
    out = subprocess.run([exe, str(tmp_path / "yolov7.onnx"), str(tmp_path / "frame.bin")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "render_test fails 0" in out.stdout
