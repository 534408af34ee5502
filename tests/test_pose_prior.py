"""Pose ambiguity without a GPU: the ABI structs and exports, every refusal the library makes before it touches the GPU,
irmv_detection_amd.pose_prior (the bit-exact host reference of the rule) on its edge cases, the C++ facade, and the
lean-back set the GPU tests run on (tests/pose_prior_set.py): on it the min-error rule reports the mirror pose and the
tilt prior the generating one -- asserted here on the mpmath reference first."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as P
import pose_prior_set as L
from conftest import ROOT
from irmv_detection_amd import _build, capi, pose_prior as pp


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def err_of(lib):
    return lib.irmv_last_error().decode()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_exports(lib):
    assert C.sizeof(capi.PosePrior) == 152 and C.sizeof(capi.PoseAlt) == 104
    assert capi.PoseAlt.err.offset == 80 and capi.PoseAlt.state.offset == 96 and capi.PosePrior.normal_up.offset == 16
    assert C.sizeof(capi.Det) == 160                                 # irmv_det stays as it is
    for name in ("irmv_engine_set_pose_prior", "irmv_engine_get_pose_prior", "irmv_engine_set_up", "irmv_engine_get_up",
                 "irmv_engine_pose_alts", "irmv_pnp_solve2"):
        assert hasattr(lib, name), name
    assert (capi.POSE_MIN_ERR, capi.POSE_PRIOR) == (pp.MIN_ERR, pp.PRIOR) == (0, 1)
    assert capi.NORMAL_UP_ROBOT == pp.NORMAL_UP_ROBOT == -math.sin(math.radians(15.0)) == -pp.NORMAL_UP_OUTPOST
    header = open(os.path.join(ROOT, "include", "irmv_hip.h")).read()
    assert "#define IRMV_POSE_MIN_ERR 0" in header and "#define IRMV_POSE_PRIOR   1" in header and "-0.25881904510252074" in header


BAD_PRIORS = [
    ("struct_size", dict(size=148), "struct_size"),
    ("struct_size0", dict(size=0), "struct_size"),
    ("mode2", dict(mode=2), "mode"),
    ("mode-1", dict(mode=-1), "mode"),
    ("ratio<1", dict(ratio=0.999), "ambiguity_ratio"),
    ("ratio0", dict(ratio=0.0), "ambiguity_ratio"),
    ("ratio-nan", dict(ratio=math.nan), "ambiguity_ratio"),
    ("ratio-neginf", dict(ratio=-math.inf), "ambiguity_ratio"),
    ("normal_up>1", dict(nu=(5, 1.0000001)), "normal_up[5]"),
    ("normal_up<-1", dict(nu=(0, -1.5)), "normal_up[0]"),
    ("normal_up-nan", dict(nu=(15, math.nan)), "normal_up[15]"),
    ("normal_up-inf", dict(nu=(7, math.inf)), "normal_up[7]"),
    ("default>1", dict(default=2.0), "normal_up_default"),
    ("default-nan", dict(default=math.nan), "normal_up_default"),
]


@pytest.mark.parametrize("case", BAD_PRIORS, ids=[c[0] for c in BAD_PRIORS])
def test_set_pose_prior_refuses_before_the_gpu(lib, case):
    """Every refusal names its field and comes before the engine is looked at (a null engine here: the GPU is never touched)."""
    _, kw, word = case
    p = capi.pose_prior_struct(kw.get("mode", capi.POSE_PRIOR), kw.get("ratio", 8.0), capi.NORMAL_UP_ROBOT, kw.get("default"))
    if "size" in kw:
        p.struct_size = kw["size"]
    if "nu" in kw:
        p.normal_up[kw["nu"][0]] = kw["nu"][1]
    assert lib.irmv_engine_set_pose_prior(None, C.byref(p)) == capi.ERR_ARG
    assert word in err_of(lib), err_of(lib)


def test_accepted_priors_reach_the_engine_check(lib):
    """The edges that are allowed -- ratio 1, ratio +inf, normal_up +-1 -- pass the value checks: the refusal is the null engine's."""
    for ratio, nu in ((1.0, 1.0), (math.inf, -1.0), (8.0, 0.0)):
        p = capi.pose_prior_struct(capi.POSE_PRIOR, ratio, nu)
        assert lib.irmv_engine_set_pose_prior(None, C.byref(p)) == capi.ERR_ARG and "engine is null" in err_of(lib)
    assert lib.irmv_engine_set_pose_prior(None, None) == capi.ERR_ARG and "engine is null" in err_of(lib)
    assert lib.irmv_engine_get_pose_prior(None, None) == capi.ERR_ARG
    n = C.c_int(0)
    assert lib.irmv_engine_pose_alts(None, 0, None, 0, C.byref(n)) == capi.ERR_ARG
    assert lib.irmv_pnp_solve2(None, None, 0, 0, None, None, None, None) == capi.ERR_ARG


BAD_UPS = [(0.0, 0.0, 0.0), (math.nan, 0.0, 1.0), (0.0, math.inf, 0.0), (-math.inf, 1.0, 1.0), (1e200, 1e200, 0.0), (0.0, -0.0, 0.0)]


@pytest.mark.parametrize("v", BAD_UPS, ids=[str(v) for v in BAD_UPS])
def test_set_up_refuses_before_the_gpu(lib, v):
    u = (C.c_double * 3)(*v)
    assert lib.irmv_engine_set_up(None, 0, u) == capi.ERR_ARG and "finite and non-zero" in err_of(lib)
    with pytest.raises(ValueError):
        pp.normalise_up(v)


def test_set_up_good_vector_reaches_the_engine_check(lib):
    u = (C.c_double * 3)(0.0, -2.0, 0.5)
    assert lib.irmv_engine_set_up(None, 0, u) == capi.ERR_ARG and "engine is null" in err_of(lib)
    assert lib.irmv_engine_set_up(None, 0, None) == capi.ERR_ARG and "up is null" in err_of(lib)
    assert lib.irmv_engine_get_up(None, 0, u) == capi.ERR_ARG


# ---- the host reference -------------------------------------------------------------------------------------------------
def test_normalise_up():
    u = pp.normalise_up((3.0, -4.0, 12.0))
    assert u.tolist() == [3.0 / 13.0, -4.0 / 13.0, 12.0 / 13.0]
    assert pp.normalise_up((0, -2, 0)).tolist() == [0.0, -1.0, 0.0]
    x, y, z = 0.1, -0.7, 0.3
    n = math.sqrt((x * x + y * y) + z * z)                      # the written association order
    assert pp.normalise_up((x, y, z)).tolist() == [x / n, y / n, z / n]


def _rot_with_normal(n0):
    """A rotation whose column 0 is the unit vector n0."""
    n0 = np.asarray(n0, np.float64) / np.linalg.norm(n0)
    a = np.cross(n0, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
    return np.stack([n0, a, np.cross(n0, a)], 1)


def test_select_edge_cases():
    u, s = np.array([0.0, -1.0, 0.0]), pp.NORMAL_UP_ROBOT
    h = math.sqrt(1.0 - s * s)
    good = _rot_with_normal([0.6 * h, -s, 0.8 * h])  # a unit normal with n . u = s up to rounding: cost ~ 0
    bad = _rot_with_normal([0.6 * h, s, 0.8 * h])    # the mirror tilt: cost = 2 |s|
    assert pp.cost(good, u, s) < 1e-15 and abs(pp.cost(bad, u, s) - 2 * abs(s)) < 1e-15
    # the plain case, both ways round, and the mode
    assert pp.select(bad, 1e-4, good, 2e-4, u, s, 8.0, pp.PRIOR) is True
    assert pp.select(good, 1e-4, bad, 2e-4, u, s, 8.0, pp.PRIOR) is False
    assert pp.select(bad, 1e-4, good, 2e-4, u, s, 8.0, pp.MIN_ERR) is False
    # ratio: errB <= ratio * errA, the edge included
    assert pp.select(bad, 1e-4, good, 8e-4, u, s, 8.0, pp.PRIOR) is True
    assert pp.select(bad, 1e-4, good, np.nextafter(8e-4, 1.0), u, s, 8.0, pp.PRIOR) is False
    # ratio = 1: B only on errB <= errA (possible: A is solution 0 unless NOT err0 <= err1, so a tie keeps 0 as A)
    assert pp.select(bad, 1e-4, good, 1e-4, u, s, 1.0, pp.PRIOR) is True
    assert pp.select(bad, 1e-4, good, np.nextafter(1e-4, 1.0), u, s, 1.0, pp.PRIOR) is False
    # ratio = inf: the cost alone -- except that inf * 0 is NaN, and NaN keeps A
    assert pp.select(bad, 1e-9, good, 1e3, u, s, math.inf, pp.PRIOR) is True
    assert pp.select(bad, 0.0, good, 1e-4, u, s, math.inf, pp.PRIOR) is False
    assert pp.select(bad, 0.0, good, 0.0, u, s, 8.0, pp.PRIOR) is True
    # equal costs keep A (strict <)
    assert pp.select(good, 1e-4, good, 1e-4, u, s, 8.0, pp.PRIOR) is False
    # any NaN keeps A
    nanR = good.copy(); nanR[1, 0] = math.nan
    for args in ((bad, math.nan, good, 1e-4), (bad, 1e-4, good, math.nan), (bad, 1e-4, nanR, 1e-4), (nanR, 1e-4, good, 1e-4)):
        assert pp.select(*args, u, s, 8.0, pp.PRIOR) is False
    assert pp.select(bad, 1e-4, good, 1e-4, np.array([0.0, math.nan, 0.0]), s, 8.0, pp.PRIOR) is False
    assert pp.select(bad, 1e-4, good, 1e-4, u, math.nan, 8.0, pp.PRIOR) is False
    assert pp.select(bad, 1e-4, good, 1e-4, u, s, math.nan, pp.PRIOR) is False


def test_cost_association_order():
    """((a + b) + c) - s, not a + (b + c): a case where the two differ in the last bit."""
    rng = np.random.default_rng(3)
    differ = 0
    for _ in range(2000):
        R = P.matrix_of(rng.normal(0, 1.5, 3))
        u = pp.normalise_up(rng.normal(0, 1, 3))
        a, b, c = R[0, 0] * u[0], R[1, 0] * u[1], R[2, 0] * u[2]
        assert pp.cost(R, u, 0.25) == abs(((a + b) + c) - 0.25)
        differ += ((a + b) + c) != (a + (b + c))
    assert differ > 50


# ---- the lean-back set --------------------------------------------------------------------------------------------------
def test_model_normal_points_away_from_the_camera():
    """Column 0 of R is the plate normal pointing AWAY from the camera: for R_FRONT it is the optical axis, and the object
    points' order LB = (0, +hy, -hz) puts model y to the left and model z up in the image."""
    assert P.R_FRONT[:, 0].tolist() == [0.0, 0.0, 1.0]
    assert P.object_points(0)[0].tolist() == [0.0, P.HALF_W[0], -P.HALF_H]
    for c in L.lean_back_set()[:40]:
        assert c["R"][2, 0] > 0 and abs(float(c["R"][:, 0] @ c["u"]) - L.S) < 1e-12      # away from the camera; leaning back 15 deg
        assert pp.cost(c["R"], c["u"], L.S) < 1e-12


def test_lean_back_set_has_its_margin_cases():
    cases = L.lean_back_set()
    kept = [c for c in cases if c["kept"]]
    margin = L.margin_cases()
    picks = sum(c["pick"] for c in kept)
    right = sum(c["pick"] and c["gen"] == 1 for c in kept)
    wrong = sum(c["pick"] != (c["gen"] == 1) for c in kept)
    print(f"lean-back set: {len(cases)} poses, {len(kept)} kept, generating pose is B in {sum(c['gen'] == 1 for c in kept)}, the rule reports B "
          f"in {picks} ({right} correctly), wrong on {wrong} of the kept")
    assert len(cases) == L.N_POSES and len(margin) >= 30
    for c in margin:                      # B is the generating pose, and the rule picks B there
        b = c["ref"]
        assert c["gen"] == 1 and b["err"][0] <= b["err"][1]
        assert np.abs(b["R"][1] - c["R"]).max() < np.abs(b["R"][0] - c["R"]).max()
        assert pp.select(b["R"][0], b["err"][0], b["R"][1], b["err"][1], c["u"], L.S, 8.0, pp.PRIOR) is True
        assert pp.select(b["R"][0], b["err"][0], b["R"][1], b["err"][1], c["u"], L.S, 8.0, pp.MIN_ERR) is False
    # the rule is not always right, and is not asserted to be: it must beat the min-error rule on the kept cases
    assert wrong < sum(c["gen"] == 1 for c in kept)


def test_quad_head_cells_do_not_overlap():
    cl = L.cells(128, 64)
    assert len(cl) == 32 and len(set(cl)) == 32
    for (ax, ay) in cl:
        for (bx, by) in cl:
            assert (ax, ay) == (bx, by) or max(abs(ax - bx), abs(ay - by)) * 8 >= 16      # 16 px boxes, centres >= 16 px apart


# ---- C++ facade -----------------------------------------------------------------------------------------------------------
def facade_exe(build=True):
    """tests/cpp/pose_prior_facade_test.cpp against the facade headers (built here so that the binary travels with the tree)."""
    bindir = os.path.join(ROOT, "tests", "cpp", "_bin")
    exe = os.path.join(bindir, "pose_prior_facade_test")
    if build or not os.path.exists(exe):
        os.makedirs(bindir, exist_ok=True)
        _build.build()
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "pose_prior_facade_test.cpp"), "-o", exe,
                               "-L", _build.LIB_DIR, "-lirmv_hip", f"-Wl,-rpath,{_build.LIB_DIR}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_facade_compiles_with_the_pose_prior_interface():
    assert subprocess.call([facade_exe()]) == 2          # without arguments: the core's parameters only, no engine
