"""Class policy, host side: the new symbols and the struct, irmv_class_policy_table / _enemy / _uniform against the numpy
reference (irmv_detection_amd.class_policy) bit for bit, every IRMV_ERR_ARG, null engines, and the C++ facade.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from irmv_detection_amd import _build, capi, class_policy
from oracle import oracle

NEW = ("irmv_engine_set_class_policy", "irmv_engine_get_class_policy", "irmv_class_policy_uniform", "irmv_class_policy_enemy",
       "irmv_class_policy_table")
F32 = np.float32
BELOW_ONE = np.nextafter(F32(1), F32(0), dtype=F32)
SUBNORMAL = F32(1.401298464324817e-45)


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def _struct(p):
    return capi.class_policy_struct(p["score_thr"], p["plate"])


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _table_rc(lib, p, nc):
    thr = (C.c_float * 16)()
    mn = C.c_float(0)
    return lib.irmv_class_policy_table(C.byref(p) if p is not None else None, nc, thr, C.byref(mn))


def test_the_new_symbols_are_bound_and_the_struct_matches_the_header(lib, tmp_path):
    names = [s[0] for s in capi.SYMBOLS]
    for sym in NEW:
        assert sym in names and hasattr(lib, sym)
    src = tmp_path / "cp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
                   "sizeof(irmv_class_policy), offsetof(irmv_class_policy, struct_size), offsetof(irmv_class_policy, score_thr), "
                   "offsetof(irmv_class_policy, plate));return 0;}\n")
    exe = tmp_path / "cp"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = capi.ClassPolicy
    assert got == [C.sizeof(P), P.struct_size.offset, P.score_thr.offset, P.plate.offset] == [84, 0, 4, 68]
    p = capi.class_policy_uniform(0.25)
    assert p.struct_size == C.sizeof(P)


@pytest.mark.parametrize("nc", [1, 14, 16])
def test_table_matches_the_numpy_reference_bit_for_bit(lib, nc):
    rng = np.random.default_rng(7)
    cases = {
        "default": class_policy.uniform(0.25),
        "half": class_policy.uniform(0.5),
        "next to 0 and 1": class_policy.policy([SUBNORMAL, BELOW_ONE, F32(1e-30), F32(1.1754944e-38), np.nextafter(BELOW_ONE, F32(0), dtype=F32),
                                                F32(0.999999), F32(1e-7)] + [0.25] * 9),
        "one and above": class_policy.policy([1.0, 0.3, 1.5, np.inf, 0.7, np.nextafter(F32(1), F32(2), dtype=F32)] + [0.25] * 10),
        "all off": class_policy.uniform(1.0),
        "random": class_policy.policy(rng.uniform(0.01, 0.99, 16).astype(F32), rng.integers(0, 2, 16)),
        "enemy blue": class_policy.enemy(0, 0.25), "enemy red": class_policy.enemy(1, 0.4, 1), "both": class_policy.enemy(-1, 0.1),
    }
    for name, p in cases.items():
        thr, mn = capi.class_policy_table(_struct(p), nc)
        ref, ref_mn = class_policy.table(p, nc)
        assert np.array_equal(_bits(thr), _bits(ref)), (name, thr, ref)
        assert _bits(mn) == _bits(ref_mn), (name, mn, ref_mn)
        assert np.all(np.isposinf(thr[nc:])) and mn == thr[:nc].min()
    # the arithmetic cfg.score_thr has: double on the float32 t, rounded once
    thr, mn = capi.class_policy_table(_struct(cases["default"]), nc)
    t = np.float64(F32(0.25))
    assert thr[0] == F32(np.log(t / (1.0 - t))) == mn
    thr, mn = capi.class_policy_table(_struct(cases["all off"]), nc)
    assert np.all(np.isposinf(thr)) and np.isposinf(mn)
    thr, _ = capi.class_policy_table(_struct(cases["one and above"]), nc)
    assert np.isposinf(thr[0]) and (nc < 6 or (np.isposinf(thr[[2, 3, 5]]).all() and np.isfinite(thr[[1, 4]]).all()))
    thr, _ = capi.class_policy_table(_struct(cases["next to 0 and 1"]), nc)
    assert np.isfinite(thr[:min(nc, 7)]).all() and thr[0] < -100


def test_bad_arguments_are_refused(lib):
    good = class_policy.uniform(0.25)
    assert _table_rc(lib, _struct(good), 14) == capi.OK
    for bad_thr in (np.nan, 0.0, -0.0, -0.25, -np.inf):
        p = class_policy.uniform(0.25)
        p["score_thr"][5] = bad_thr
        assert _table_rc(lib, _struct(p), 14) == capi.ERR_ARG, bad_thr
        assert b"score_thr[5]" in lib.irmv_last_error()
        assert _table_rc(lib, _struct(p), 5) == capi.OK          # entries at and above nc are ignored
        with pytest.raises(ValueError):
            class_policy.table(p, 14)
    for bad_plate in (2, 255):
        p = class_policy.uniform(0.25)
        p["plate"][13] = bad_plate
        assert _table_rc(lib, _struct(p), 14) == capi.ERR_ARG
        assert _table_rc(lib, _struct(p), 13) == capi.OK
        with pytest.raises(ValueError):
            class_policy.table(p, 14)
    s = _struct(good)
    for size in (0, 4, C.sizeof(capi.ClassPolicy) - 1, C.sizeof(capi.ClassPolicy) + 4):
        s.struct_size = size
        assert _table_rc(lib, s, 14) == capi.ERR_ARG
    assert _table_rc(lib, None, 14) == capi.ERR_ARG
    s = _struct(good)
    mn = C.c_float(0)
    thr = (C.c_float * 16)()
    assert lib.irmv_class_policy_table(C.byref(s), 14, None, C.byref(mn)) == capi.ERR_ARG
    assert lib.irmv_class_policy_table(C.byref(s), 14, thr, None) == capi.ERR_ARG
    for nc in (0, -1, 17):
        assert _table_rc(lib, s, nc) == capi.ERR_ARG
    out = capi.ClassPolicy()
    for c in (-2, 2, 7):
        assert lib.irmv_class_policy_enemy(c, 0.25, capi.ARMOR_SMALL, C.byref(out)) == capi.ERR_ARG
        with pytest.raises(ValueError):
            class_policy.enemy(c)
    assert lib.irmv_class_policy_enemy(0, 0.25, capi.ARMOR_SMALL, None) == capi.ERR_ARG
    assert lib.irmv_class_policy_enemy(0, 0.25, 2, C.byref(out)) == capi.ERR_ARG
    assert lib.irmv_class_policy_enemy(0, float("nan"), capi.ARMOR_SMALL, C.byref(out)) == capi.ERR_ARG
    assert lib.irmv_class_policy_uniform(0.0, capi.ARMOR_SMALL, C.byref(out)) == capi.ERR_ARG
    assert lib.irmv_class_policy_uniform(0.25, capi.ARMOR_SMALL, None) == capi.ERR_ARG


def test_enemy_follows_the_armor_class_order_of_the_facade(lib):
    text = open(os.path.join(ROOT, "include", "irmv_detection", "armor.hpp")).read()
    order = re.findall(r"X\((\w+)\)", re.search(r"#define IRMV_ARMOR_CLASS_LIST\(X\)(.*)", text).group(1))
    assert len(order) == 14
    blue = [i for i, n in enumerate(order) if n.startswith("B")]
    red = [i for i, n in enumerate(order) if n.startswith("R")]
    assert blue == list(class_policy.BLUE) and red == list(class_policy.RED)
    from irmv_detection_amd.engine import ArmorClass
    assert [c.name for c in ArmorClass][:14] == order
    for colour, on, off in ((0, blue, red), (1, red, blue), (-1, blue + red, [])):
        p = capi.class_policy_enemy(colour, 0.3, capi.ARMOR_LARGE)
        thr = np.array(p.score_thr[:], F32)
        assert np.all(thr[on] == F32(0.3)) and np.all(thr[off] >= 1) and np.all(thr[14:] == F32(0.3))
        assert list(p.plate) == [capi.ARMOR_LARGE] * 16
        ref = class_policy.enemy(colour, 0.3, capi.ARMOR_LARGE)
        assert np.array_equal(_bits(thr), _bits(ref["score_thr"])) and np.array_equal(np.array(p.plate[:]), ref["plate"])
        logit, _ = capi.class_policy_table(p, 14)
        assert np.isfinite(logit[on]).all() and np.isposinf(logit[off]).all()
    u = capi.class_policy_uniform(0.3, capi.ARMOR_LARGE)
    b = capi.class_policy_enemy(-1, 0.3, capi.ARMOR_LARGE)
    assert bytes(u) == bytes(b)


def test_erase_states_the_policy_on_a_head():
    nc, nk = 14, 8
    rng = np.random.default_rng(3)
    head = rng.standard_normal((50, 64 + nc + nk)).astype(F32) * 3
    p = class_policy.enemy(0, 0.25)
    p["score_thr"][2] = 0.9
    thr, mn = class_policy.table(p, nc)
    e = class_policy.erase(head, p, nc)
    cl, ecl = head[:, 64:64 + nc], e[:, 64:64 + nc]
    keep = cl > thr[:nc]
    assert keep.any() and not keep[:, 7:].any() and np.array_equal(keep, class_policy.passes(head, p, nc))
    assert np.array_equal(ecl[keep], cl[keep]) and np.all(ecl[~keep] == class_policy.DARK)
    assert np.array_equal(e[:, :64], head[:, :64]) and np.array_equal(e[:, 64 + nc:], head[:, 64 + nc:])
    assert np.array_equal(ecl > mn, keep)           # decoding the erased head at the smallest enabled threshold gives the policy's list
    assert class_policy.min_score_thr(p, nc) == float(F32(0.25)) and class_policy.min_score_thr(class_policy.uniform(1.0), nc) is None
    import detect_craft
    assert class_policy.DARK == detect_craft.DARK


# ---- the density table of tests/test_gpu_class_policy.py ---------------------------------------------------------------------
def density_policy():
    """The blue mask (R1..RS off) plus one raised threshold."""
    pol = class_policy.enemy(0, 0.25)
    pol["score_thr"][2] = np.float32(0.6)
    return pol


MASKED_NC = 7          # classes the density policy leaves on: the bands' "all" is A * 7 pairs
# 416 x 416, class finals shifted by delta: (delta, (frame per slot), (band of detect_craft.bands per slot)) for the candidate
# count UNDER density_policy().  The mask roughly halves test_detect_craft.DENSITY's counts, so the deltas are this table's
# own.  CPU oracle: +0.25 -> 0, 15, 15, 30; +3.25 -> 878, 884, 683, 750; +4.5 -> 1843, 2179, 1705, 1724;
# +6 -> 5727, 5270, 5340, 5275; +7.75 -> 12236, 13688, 12263, 11939; +30 -> 24843 = 7 A each.
MASKED_DENSITY = [(0.25, (3, 0, 10, 15), ("0", "1-64", "1-64", "1-64")),
                  (3.25, (0, 2, 3, 6), ("513-1024",) * 4),
                  (4.5, (0, 1, 4, 5), ("1025-4096",) * 4),
                  (6.0, (1, 3, 6, 11), ("4097-8192",) * 4),
                  (7.75, (0, 1, 2, 4), (">8192",) * 4),
                  (30.0, (0, 1, 2, 3), ("all",) * 4)]


def test_masked_density_table_sits_inside_its_bands(blob):
    """The CPU oracle's count of the erased head of every (delta, frame) pair sits inside its band with a fifth of the
    band's width clear of either edge (the GPU's fp16 head moves a count by a few per cent), and the table reaches every band."""
    import detect_craft as dc
    from test_detect_craft import oracle_head
    W = H = 416
    A = sum(dc.level_sizes(W, H))
    pol = density_policy()
    assert {b for _, _, want in MASKED_DENSITY for b in want} == set(dc.bands(A, MASKED_NC))
    heads = {}
    for delta, fr, want in MASKED_DENSITY:
        for f, band in zip(fr, want):
            if f not in heads:
                heads[f] = oracle_head(blob, W, H, f)
            h = heads[f].copy()
            h[:, 64:78] += np.float32(delta)
            n = int(class_policy.passes(h, pol, 14).sum())
            ref = oracle.decode_nms(class_policy.erase(h, pol, 14), W, 14, 8, score_thr=class_policy.min_score_thr(pol, 14))
            assert ref["n_candidates"] == n
            lo, hi = dc.bands(A, MASKED_NC)[band]
            assert dc.inside_with_margin(n, lo, hi), (delta, f, n, band)


def test_null_engines_are_refused(lib):
    p = capi.class_policy_uniform(0.25)
    assert lib.irmv_engine_set_class_policy(None, C.byref(p)) == capi.ERR_ARG
    assert lib.irmv_engine_set_class_policy(None, None) == capi.ERR_ARG
    assert lib.irmv_engine_get_class_policy(None, C.byref(p)) == capi.ERR_ARG


FACADE_SRC = r"""
#include <cstdio>
#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/yolo_engine.hpp"

using irmv_detection::ArmorClass;
using irmv_detection::IrmDetectorCore;
using irmv_detection::YoloEngine;

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  YoloEngine engine(argv[1], cv::Size(1280, 1024), true);
  engine.set_enemy_color(1);                      // the enemy is red: blue armour costs nothing behind the class carriers
  irmv_class_policy p = engine.user_class_policy();
  p.plate[int(ArmorClass::R1)] = IRMV_ARMOR_LARGE;   // this season's hero plate
  p.score_thr[int(ArmorClass::RS)] = 0.6f;           // the sentry fires on less
  engine.set_class_policy(p);                        // the colour stays in force
  auto bboxes = engine.detect();
  engine.set_enemy_color(0);                         // the referee says otherwise: RS keeps its 0.6 for when red is on again
  const irmv_class_policy in_force = engine.class_policy();
  engine.set_class_policy(p, -1);                    // policy and colour in one upload
  engine.reset_class_policy();
  if (in_force.score_thr[0] >= 1.f || engine.enemy_color() != -1) return 3;

  IrmDetectorCore::Params params;
  params.enemy_color = 0;
  params.large_plate_classes = {int(ArmorClass::B1), int(ArmorClass::R1)};
  IrmDetectorCore core(argv[1], {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1}, {-0.405274, 0.126058, -0.026939, -0.006503, 0.0}, params);
  const bool ok = core.set_parameter("enemy_color", 1);          // the referee system announces the colour
  const bool bad = core.set_parameter("enemy_color", 3);
  std::printf("bboxes %zu accepted %d refused %d colour %d\n", bboxes.size(), ok ? 1 : 0, bad ? 0 : 1, core.params().enemy_color);
  return 0;
}
"""


def test_reference_style_policy_code_compiles_against_the_facade():
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    os.makedirs(bindir, exist_ok=True)
    src = os.path.join(bindir, "class_policy_facade_test.cpp")
    with open(src, "w") as f:
        f.write(FACADE_SRC)
    exe = os.path.join(bindir, "class_policy_facade_test")
    _build.build()
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    assert os.path.exists(exe)
