"""Shared by tests/test_bayer_isp.py and tests/test_gpu_bayer_isp.py: a second reference of the Malvar-He-Cutler demosaic
written by the letter (per pixel, the four 5 x 5 masks as literal tables in eighths, exact rationals), the gamma LUT the
tests use, and the facade program of the compile and run tests."""
import os
import subprocess
from fractions import Fraction as F

import numpy as np

from conftest import ROOT
from irmv_detection_amd import _build

H2 = F(1, 2)
# rows N2 .. S2, columns W2 .. E2, in units of 1/8 (Malvar, He, Cutler 2004, figure 2)
G_AT_RB = [[0, 0, -1, 0, 0],
           [0, 0, 2, 0, 0],
           [-1, 2, 4, 2, -1],
           [0, 0, 2, 0, 0],
           [0, 0, -1, 0, 0]]
IN_ROW = [[0, 0, H2, 0, 0],        # at a G site, the colour whose samples are this site's W / E neighbours
          [0, -1, 0, -1, 0],
          [-1, 4, 5, 4, -1],
          [0, -1, 0, -1, 0],
          [0, 0, H2, 0, 0]]
IN_COL = [[0, 0, -1, 0, 0],        # ... and the one whose samples are its N / S neighbours
          [0, -1, 4, -1, 0],
          [H2, 0, 5, 0, H2],
          [0, -1, 4, -1, 0],
          [0, 0, -1, 0, 0]]
OPPOSITE = [[0, 0, -3 * H2, 0, 0],  # B at an R site, R at a B site
            [0, 2, 0, 2, 0],
            [-3 * H2, 0, 6, 0, -3 * H2],
            [0, 2, 0, 2, 0],
            [0, 0, -3 * H2, 0, 0]]
RED_PHASE = {"RGGB": (0, 0), "BGGR": (1, 1), "GRBG": (0, 1), "GBRG": (1, 0)}


def _reflect(i, n):
    """-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3"""
    if i == -1:
        return 1
    if i == -2:
        return 2
    if i == n:
        return n - 2
    if i == n + 1:
        return n - 3
    assert 0 <= i < n
    return i


def mhc_unclamped(raw, pattern):
    """[H][W][3] python ints: floor(x + 1/2) of the exact filter value x, BEFORE the clamp to [0, 255]."""
    H, W = raw.shape
    ry, rx = RED_PHASE[pattern]

    def filt(mask, y, x):
        s = F(0)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                s += F(mask[dy + 2][dx + 2]) * int(raw[_reflect(y + dy, H), _reflect(x + dx, W)])
        v = s / 8 + H2
        return v.numerator // v.denominator          # floor

    out = np.zeros((H, W, 3), np.int64)
    for y in range(H):
        for x in range(W):
            c = int(raw[y, x])
            r_row, r_col = (y & 1) == ry, (x & 1) == rx
            if r_row and r_col:
                out[y, x] = (c, filt(G_AT_RB, y, x), filt(OPPOSITE, y, x))
            elif not r_row and not r_col:
                out[y, x] = (filt(OPPOSITE, y, x), filt(G_AT_RB, y, x), c)
            elif r_row:                              # G on an R row: R from W / E, B from N / S
                out[y, x] = (filt(IN_ROW, y, x), c, filt(IN_COL, y, x))
            else:
                out[y, x] = (filt(IN_COL, y, x), c, filt(IN_ROW, y, x))
    return out


def mhc_by_the_letter(raw, pattern):
    return np.clip(mhc_unclamped(raw, pattern), 0, 255).astype(np.uint8)


def apply_gain(v, g):
    """k_bayer.hip's apply_gain in python ints."""
    return min(255, (v * g + 128) >> 8)


def gamma_lut(gamma=0.5):
    return np.array([int(255.0 * (v / 255.0) ** gamma + 0.5) for v in range(256)], np.uint8)


GAINS = (300, 256, 410)

# Reference-style code on the facade: an MHC engine on the camera's raw buffer, retuned while it lives.  Prints the
# detections before and after the set, floats in hex.
FACADE_SRC = r"""
#include <cstdio>
#include <vector>
#include "irmv_detection/yolo_engine.hpp"

static void print(const char * tag, const std::vector<irmv_detection::YoloEngine::bbox> & bb)
{
  std::printf("%s %zu\n", tag, bb.size());
  for (const auto & b : bb)
    std::printf("%s %a %a %a %a %a %d\n", tag, b.xyxy[0], b.xyxy[1], b.xyxy[2], b.xyxy[3], b.score, static_cast<int>(b.class_id));
}

int main(int argc, char ** argv)
{
  if (argc < 4) return 2;
  irmv_detection::YoloEngine engine(argv[1], cv::Size(1280, 1024), true, -1, false, -1, IRMV_SRC_BAYER_GRBG8, {256, 256, 256}, -1,
                                    IRMV_DEMOSAIC_MHC);
  FILE * f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  const size_t n = std::fread(engine.get_src_image_buffer(), 1, engine.src_image_bytes(), f);
  std::fclose(f);
  if (n != engine.src_image_bytes()) return 4;
  std::vector<uint8_t> lut(768);
  f = std::fopen(argv[3], "rb");
  if (!f || std::fread(lut.data(), 1, 768, f) != 768) return 5;
  std::fclose(f);
  print("before", engine.detect());
  engine.set_bayer_isp({300, 256, 410}, lut.data());
  print("after", engine.detect());
  engine.set_bayer_isp({256, 256, 256});
  print("back", engine.detect());
  return 0;
}
"""


def facade_exe():
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    os.makedirs(bindir, exist_ok=True)
    src = os.path.join(bindir, "bayer_isp_facade_test.cpp")
    with open(src, "w") as f:
        f.write(FACADE_SRC)
    exe = os.path.join(bindir, "bayer_isp_facade_test")
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe
