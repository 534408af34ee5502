"""Frame metering through the C++ facade and the detector core's automatic white balance (tests/cpp/metering_test.cpp):
compiled here like the programs of tests/test_cpp_facade.py (so the binary travels to the GPU box with the tree), run on the
GPU against a record that irmv_detection_amd/metering.py writes beside the frame."""
import ctypes as C
import os
import subprocess

import pytest

import detect_craft as dc
from conftest import ROOT
from irmv_detection_amd import _build, capi, metering
from test_metering import tinted_scene

INC = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "_bin")
EXE = os.path.join(BIN, "metering_test")


def _compile():
    os.makedirs(BIN, exist_ok=True)
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", INC, os.path.join(CPP, "metering_test.cpp"), "-o", EXE,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


def test_metering_program_compiles_against_the_facade():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_facade_and_core_meter_on_gpu(tmp_path, blob):
    exe = EXE if os.path.exists(EXE) else _compile()
    crafted = dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))   # detections on every frame
    (tmp_path / "yolov7.irmw").write_bytes(crafted)
    raw = tinted_scene("RGGB")
    raw.tofile(tmp_path / "frame.bin")
    rec = metering.meter(raw, None, 1, "raw", True, "RGGB")
    (tmp_path / "stats.bin").write_bytes(bytes(capi.stats_struct(rec)))
    assert os.path.getsize(tmp_path / "stats.bin") == C.sizeof(capi.FrameStats)
    gains = metering.gray_world(rec, 8, 247)
    out = subprocess.run([exe, str(tmp_path / "yolov7.onnx"), str(tmp_path / "frame.bin"), str(tmp_path / "stats.bin"), str(gains[0]), str(gains[2])],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "metering_test fails 0" in out.stdout
