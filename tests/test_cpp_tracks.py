"""Armor tracks through the C++ facade and the detector core (tests/cpp/tracks_facade_test.cpp): compiled here like the programs
of tests/test_cpp_facade.py (so the binary travels to the GPU box with the tree), run on the GPU; the records the program saw at
every step are then compared with the host reference fed the program's own detections."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import detect_craft as dc
import patch_set as PS
import track_set as TS
from conftest import ROOT
from irmv_detection_amd import _build, capi, tracks as T

INC = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "_bin")
EXE = os.path.join(BIN, "tracks_facade_test")


def _compile():
    os.makedirs(BIN, exist_ok=True)
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", INC, os.path.join(CPP, "tracks_facade_test.cpp"), "-o", EXE,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


def test_tracks_program_compiles_against_the_facade():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_facade_and_core_deliver_tracks_on_gpu(tmp_path, blob):
    exe = EXE if os.path.exists(EXE) else _compile()
    crafted = dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))   # detections on every frame
    (tmp_path / "yolov7.irmw").write_bytes(crafted)
    PS.to_buffer(PS.step_frame(0), True).tofile(tmp_path / "frame.bin")
    out = subprocess.run([exe, str(tmp_path / "yolov7.onnx"), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "tracks_facade_test fails 0" in out.stdout
    data = (tmp_path / "out.bin").read_bytes()
    steps, at = struct.unpack_from("<i", data, 0)[0], 4
    assert steps == 4
    ref = T.Tracker()
    sd = C.sizeof(capi.Det)
    matched = 0
    for k in range(steps):
        n, t, *tw = struct.unpack_from("<id3d", data, at)
        at += 36
        dets = [capi.Det.from_buffer_copy(data, at + i * sd) for i in range(n)]
        at += n * sd
        got = data[at:at + n * T.DET_TRACK_SIZE], data[at + n * T.DET_TRACK_SIZE:at + n * T.DET_TRACK_SIZE + T.FRAME_SIZE]
        at += n * T.DET_TRACK_SIZE + T.FRAME_SIZE
        snap = data[at:at + 32 * T.TRACK_SIZE]
        at += 32 * T.TRACK_SIZE
        obs = [T.Obs(d.class_id, tuple(d.tvec), 1 if (d.pnp_ok == 1 and d.armor_valid == 1) else 0) for d in dets]
        res = ref.update(t, obs, T.IDENTITY, tuple(tw))
        want = TS.pack_result(res)
        assert (got[0], got[1], snap) == want, k
        matched += sum(d.state == T.DET_MATCHED for d in res[0])
    assert at == len(data) and n >= 1 and matched >= 1
