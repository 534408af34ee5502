"""The pose uncertainty through the C++ facade and the detector core (tests/cpp/pose_cov_facade_test.cpp): compiled here like
the programs of tests/test_cpp_facade.py (so the binary travels to the GPU box with the tree), run on the GPU; the records the
program saw are then compared with the C ABI's through the Python binding and with the host reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detect_craft as dc
import patch_set as PS
import pose_cov_set as S
from conftest import ROOT
from irmv_detection_amd import _build, capi, pose_cov as pc, yaw_solve as ys

INC = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "_bin")
EXE = os.path.join(BIN, "pose_cov_facade_test")


def _compile():
    os.makedirs(BIN, exist_ok=True)
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", INC, os.path.join(CPP, "pose_cov_facade_test.cpp"), "-o", EXE,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return EXE


def test_pose_cov_program_compiles_against_the_facade():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_facade_and_core_deliver_pose_covs_on_gpu(tmp_path, blob):
    exe = EXE if os.path.exists(EXE) else _compile()
    crafted = dc.craft(blob, cls=("bias", dc.two_tied_bias(14)), kpt=("bias", dc.quad_kpt_bias(8)))   # detections on every frame
    (tmp_path / "yolov7.irmw").write_bytes(crafted)
    frame = PS.to_buffer(PS.step_frame(0), True)
    frame.tofile(tmp_path / "frame.bin")
    out = subprocess.run([exe, str(tmp_path / "yolov7.onnx"), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "pose_cov_facade_test fails 0" in out.stdout
    data = (tmp_path / "out.bin").read_bytes()
    n = int.from_bytes(data[:4], "little")
    sd, sy, sc = C.sizeof(capi.Det), C.sizeof(capi.YawPose), C.sizeof(capi.PoseCov)
    assert n >= 1 and len(data) == 4 + n * (sd + sy + sc)
    dets = [capi.Det.from_buffer_copy(data, 4 + i * sd) for i in range(n)]
    yaws = [capi.YawPose.from_buffer_copy(data, 4 + n * sd + i * sy) for i in range(n)]
    covs = [capi.PoseCov.from_buffer_copy(data, 4 + n * (sd + sy) + i * sc) for i in range(n)]
    # the host reference on the program's own records
    from irmv_detection_amd.engine import DEFAULT_CAMERA_MATRIX, DEFAULT_DIST_COEFFS, YoloEngine
    cam = ys.camera_of(DEFAULT_CAMERA_MATRIX, DEFAULT_DIST_COEFFS)
    seen = 0
    for d, y, c in zip(dets, yaws, covs):
        if not (d.pnp_ok == 1 and d.armor_valid == 1):
            assert bytes(c) == bytes(capi.PoseCov())
            continue
        yaw = (list(y.rvec), list(y.tvec), (0.0, -1.0, 0.0)) if y.state == 1 else None
        ref = pc.pose_cov(cam, np.array(list(d.kpts), np.float32), d.armor_size, list(d.rvec), list(d.tvec), 0.5, yaw=yaw)
        assert S.same_bits(c, ref), S.first_difference(c, ref)
        seen += c.state == 1
    assert seen >= 1
    # the C ABI's records of the same frame, through the Python binding
    with YoloEngine(None, PS.SRC, weights_blob=crafted, net_size=64) as e:
        e.set_yaw_solve()
        e.set_pose_cov(sigma_px=0.5)
        e.get_src_image_buffer()[:] = frame
        e.detect()
        assert [bytes(c) for c in e.pose_covs(0)] == [bytes(c) for c in covs]
