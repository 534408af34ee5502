"""Share of (tile, image) pairs that hold a candidate anchor, per gated kernel's own tile shape ("Sparse
branch"): the CPU oracle with emulate_fp16 on the benchmark's frames 0 .. N-1, synthetic blob 0, score threshold 0.25.

    python3 scripts/sparse_branch_activity.py [N=256] > profiles/sparse_branch_activity.txt

active: mean over (tile, image).  worst: a workgroup keeps a tile position for `ipw` consecutive images (of a 128-frame graph),
and the launch lasts as long as its slowest workgroup -- the largest active share of any (tile position, image group), averaged
over the image groups: what a gated launch run alone can fall to at best.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irmv_detection_amd import frames, weights  # noqa: E402
from oracle import oracle  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
THR = np.log(0.25 / 0.75)


def grow(m, halo):
    if not halo:
        return m
    H, W = m.shape
    p, d = np.pad(m, halo), np.zeros_like(m)
    for dy in range(2 * halo + 1):
        for dx in range(2 * halo + 1):
            d |= p[dy:dy + H, dx:dx + W]
    return d


def blocks(m, th, tw, halo):     # 2-D tiles: active if a candidate lies in the tile grown by the halo
    H, W = m.shape
    m = grow(m, halo)
    ny, nx = -(-H // th), -(-W // tw)
    p = np.zeros((ny * th, nx * tw), bool)
    p[:H, :W] = m
    return p.reshape(ny, th, nx, tw).any(axis=(1, 3)).reshape(-1)


def runs(m, px, halo):           # row runs: the run of px anchors, grown by a row and a pixel each way
    f, r = m.reshape(-1), halo * (m.shape[1] + 1)
    return np.array([f[max(k - r, 0):k + px + r].any() for k in range(0, f.size, px)])


# (label, level, images per workgroup at 128 frames, activity of one image's candidate map)
KERNELS = [
    ("kpt3 80x80, 10x10 tiles", 0, 8, lambda m: blocks(m, 10, 10, 0)),
    ("kpt3 40x40, 10x10 tiles", 1, 2, lambda m: blocks(m, 10, 10, 0)),
    ("kpt3 20x20, 10x10 tiles", 2, 1, lambda m: blocks(m, 10, 10, 0)),
    ("cv2.0.1 + final 80x80, ping-pong 8x16 blocks, halo 0", 0, 13, lambda m: blocks(m, 8, 16, 0)),
    ("cv2.0.0 80x80, ping-pong 8x16 blocks, halo 1", 0, 13, lambda m: blocks(m, 8, 16, 1)),
    ("cv2.1.1 + final 40x40, runs of 256 anchors, halo 0", 1, 1, lambda m: runs(m, 256, 0)),
    ("cv2.2.1 + final 20x20, runs of 256 anchors, halo 0", 2, 1, lambda m: runs(m, 256, 0)),
]

oracle.build()
net = oracle.Net(weights.synthetic_blob(0))
nc = net.nc
maps, per_frame, empty = [], [], [0, 0, 0]
for i in range(N):
    head = net.forward(oracle.preprocess(frames.synthetic_frame(i), 640), emulate_fp16=True)
    a = (head[:, 64:64 + nc] > THR).any(1)
    lv = [a[:6400].reshape(80, 80), a[6400:8000].reshape(40, 40), a[8000:].reshape(20, 20)]
    maps.append(lv)
    per_frame.append(int(a.sum()))
    for l in range(3):
        empty[l] += int(not lv[l].any())
print(f"frames 0 .. {N - 1}: candidate anchors per frame mean {np.mean(per_frame):.0f}, median {np.median(per_frame):.0f}, max {max(per_frame)};"
      f" frames without a candidate on the 80x80 / 40x40 / 20x20 level: {empty[0]} / {empty[1]} / {empty[2]}")
print(f"{'gated launch, tile':58s} {'tiles':>5s} {'ipw':>3s} {'active':>6s} {'worst':>6s}")
for label, l, ipw, act in KERNELS:
    v = np.stack([act(m[l]) for m in maps])          # [N, tiles]
    worst = []
    for h0 in range(0, N, 128):                      # the benchmark's graphs hold 128 consecutive frames
        half = v[h0:h0 + 128]
        for g in range(0, len(half), ipw):
            worst.append(half[g:g + ipw].mean(0).max())
    print(f"{label:58s} {v.shape[1]:5d} {ipw:3d} {v.mean():6.3f} {np.mean(worst):6.3f}")
