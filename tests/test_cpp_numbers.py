"""Plate numbers through the C++ facade and the detector core (tests/cpp/number_facade_test.cpp): compiled here like the
programs of tests/test_cpp_facade.py (so the binary travels to the GPU box with the tree), run on the GPU with an .irmn model
that irmv_detection_amd/number_net.py writes; the records the program saw are then compared with the C ABI's through the
Python binding and with the host reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detect_craft as dc
import patch_set as PS
from conftest import ROOT
from irmv_detection_amd import _build, capi, number_net as NN

INC = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "_bin")
EXE = os.path.join(BIN, "number_facade_test")


def _compile():
    os.makedirs(BIN, exist_ok=True)
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", INC, os.path.join(CPP, "number_facade_test.cpp"), "-o", EXE,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


def test_number_program_compiles_against_the_facade():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_facade_and_core_read_numbers_on_gpu(tmp_path, blob):
    exe = EXE if os.path.exists(EXE) else _compile()
    crafted = dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))   # detections on every frame
    (tmp_path / "yolov7.irmw").write_bytes(crafted)
    frame = PS.to_buffer(PS.step_frame(0), True)
    frame.tofile(tmp_path / "frame.bin")
    r = np.random.RandomState(31)
    model = NN.NumberModel([(r.standard_normal((64, 560)) / 24).astype(np.float32), (r.standard_normal((9, 64)) / 8).astype(np.float32)],
                           [(r.standard_normal(64) * 0.3).astype(np.float32), (r.standard_normal(9) * 0.3).astype(np.float32)])
    model.save(str(tmp_path / "numbers.irmn"))
    out = subprocess.run([exe, str(tmp_path / "yolov7.onnx"), str(tmp_path / "frame.bin"), str(tmp_path / "numbers.irmn"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "number_facade_test fails 0" in out.stdout
    data = (tmp_path / "out.bin").read_bytes()
    n = int.from_bytes(data[:4], "little")
    assert n >= 1 and len(data) == 4 + n * (C.sizeof(capi.PlatePatch) + C.sizeof(capi.PlateNumber))
    patches = [capi.PlatePatch.from_buffer_copy(data, 4 + i * 592) for i in range(n)]
    numbers = np.frombuffer(data, NN.NUMBER_DTYPE, n, 4 + n * 592)
    assert numbers.tobytes() == model.reference(patches).tobytes() and (numbers["state"] == 1).sum() >= 1
    # the C ABI's records of the same frame, through the Python binding
    from irmv_detection_amd.engine import YoloEngine
    with YoloEngine(None, PS.SRC, weights_blob=crafted, net_size=64) as e:
        e.set_number_model(str(tmp_path / "numbers.irmn"))
        e.set_numbers()
        e.get_src_image_buffer()[:] = frame
        e.detect()
        assert [bytes(p) for p in e.plate_patches(0)] == [bytes(p) for p in patches]
        assert NN.records(e.plate_numbers(0)).tobytes() == numbers.tobytes()
