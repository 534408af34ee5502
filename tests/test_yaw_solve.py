"""The constrained pose without a GPU (include/irmv_hip.h, "constrained pose"): the ABI structs and exports, every refusal the
library makes before it touches the GPU, irmv_detection_amd.yaw_solve (the host reference of the model and the grid walk) on
its own properties, and the yaw-error statistics of the lean-back set (tests/pose_prior_set.py) beside the min-error rule and
the gravity prior."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as P
import pose_prior_set as L
import yaw_set as YS
from conftest import ROOT
from irmv_detection_amd import _build, capi, yaw_solve as Y


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def err_of(lib):
    return lib.irmv_last_error().decode()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_exports(lib, tmp_path):
    assert C.sizeof(capi.YawOpts) == 32 and C.sizeof(capi.YawPose) == 144
    for name in ("irmv_engine_set_yaw_solve", "irmv_engine_get_yaw_solve", "irmv_engine_yaw_poses", "irmv_pnp_solve_yaw"):
        assert hasattr(lib, name), name
    parts = ['printf("%zu %zu %zu %zu %zu", sizeof(irmv_yaw_opts), sizeof(irmv_yaw_pose), sizeof(irmv_det), sizeof(irmv_pose_alt), sizeof(irmv_tile_det));']
    parts += [f'printf(" %zu", offsetof(irmv_yaw_opts, {f}));' for f, _ in capi.YawOpts._fields_]
    parts += [f'printf(" %zu", offsetof(irmv_yaw_pose, {f}));' for f, _ in capi.YawPose._fields_]
    src = tmp_path / "yw.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(parts) + "return 0;}\n")
    exe = tmp_path / "yw"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == ([32, 144, 160, 104, C.sizeof(capi.TileDet)] + [getattr(capi.YawOpts, f).offset for f, _ in capi.YawOpts._fields_] +
                   [getattr(capi.YawPose, f).offset for f, _ in capi.YawPose._fields_])      # (irmv_det and irmv_pose_alt stay as they are)


BAD_OPTS = [
    ("struct_size", dict(size=28), "struct_size"),
    ("struct_size0", dict(size=0), "struct_size"),
    ("enable2", dict(enable=2), "enable"),
    ("enable-1", dict(enable=-1), "enable"),
    ("rounds0", dict(rounds=0), "rounds"),
    ("rounds7", dict(rounds=7), "rounds"),
    ("reserved", dict(reserved=1), "reserved"),
    ("tau_max0", dict(tau_max=0.0), "tau_max"),
    ("tau_max>4", dict(tau_max=4.0000001), "tau_max"),
    ("tau_max-neg", dict(tau_max=-1.0), "tau_max"),
    ("tau_max-nan", dict(tau_max=math.nan), "tau_max"),
    ("tau_max-inf", dict(tau_max=math.inf), "tau_max"),
    ("horizon0", dict(horizon_min=0.0), "horizon_min"),
    ("horizon1", dict(horizon_min=1.0), "horizon_min"),
    ("horizon-nan", dict(horizon_min=math.nan), "horizon_min"),
]


def _opts(kw):
    o = capi.yaw_opts_struct(kw.get("enable", 1), kw.get("rounds", 4), kw.get("tau_max", 1.0), kw.get("horizon_min", 1e-4))
    if "size" in kw:
        o.struct_size = kw["size"]
    o.reserved = kw.get("reserved", 0)
    return o


@pytest.mark.parametrize("case", BAD_OPTS, ids=[c[0] for c in BAD_OPTS])
def test_set_yaw_solve_refuses_before_the_gpu(lib, case):
    """Every refusal names its field and comes before the engine is looked at (a null engine here: the GPU is never touched);
    the stand-alone call makes the same checks."""
    _, kw, word = case
    o = _opts(kw)
    assert lib.irmv_engine_set_yaw_solve(None, C.byref(o)) == capi.ERR_ARG
    assert word in err_of(lib), err_of(lib)


def test_accepted_opts_reach_the_engine_check(lib):
    for kw in (dict(rounds=1), dict(rounds=6), dict(tau_max=4.0), dict(tau_max=1e-3), dict(horizon_min=0.999), dict(enable=0)):
        assert lib.irmv_engine_set_yaw_solve(None, C.byref(_opts(kw))) == capi.ERR_ARG and "engine is null" in err_of(lib)
    assert lib.irmv_engine_set_yaw_solve(None, None) == capi.ERR_ARG and "opts is null" in err_of(lib)
    assert lib.irmv_engine_get_yaw_solve(None, None) == capi.ERR_ARG
    n = C.c_int(0)
    assert lib.irmv_engine_yaw_poses(None, 0, None, 0, C.byref(n)) == capi.ERR_ARG


SOLVE_OPTS = [c for c in BAD_OPTS if "enable" not in c[1]]      # (irmv_pnp_solve_yaw does not read enable)


@pytest.mark.parametrize("case", SOLVE_OPTS, ids=[c[0] for c in SOLVE_OPTS])
def test_solve_yaw_refuses_the_same_opts(lib, case):
    _, kw, word = case
    assert _solve_yaw(lib, opts=_opts(kw)) == capi.ERR_ARG and word in err_of(lib), err_of(lib)


def _solve_yaw(lib, up=(0.0, -1.0, 0.0), normal_up=0.0, size=0, opts=None, n=1, pts=True, out=True, upp=True):
    """irmv_pnp_solve_yaw on a null solver: every value check comes before the solver is looked at."""
    o = _opts({}) if opts is None else opts
    return lib.irmv_pnp_solve_yaw(None, (C.c_float * 8)() if pts else None, n, size, (C.c_double * 3)(*up) if upp else None, normal_up,
                                  C.byref(o), (capi.YawPose * 1)() if out else None)


SOLVE_BAD = [
    ("normal_up>1", dict(normal_up=1.0000001), "normal_up"),
    ("normal_up<-1", dict(normal_up=-1.5), "normal_up"),
    ("normal_up-nan", dict(normal_up=math.nan), "normal_up"),
    ("up-zero", dict(up=(0.0, 0.0, 0.0)), "up must be"),
    ("up-nan", dict(up=(0.0, math.nan, 1.0)), "up must be"),
    ("up-inf", dict(up=(math.inf, 0.0, 0.0)), "up must be"),
    ("up-overflow", dict(up=(1e200, 1e200, 0.0)), "up must be"),
    ("armor_size2", dict(size=2), "armor_size"),
    ("armor_size-1", dict(size=-1), "armor_size"),
    ("n<0", dict(n=-1), "null argument"),
    ("pts-null", dict(pts=False), "null argument"),
    ("up-null", dict(upp=False), "null argument"),
    ("out-null", dict(out=False), "null argument"),
]


@pytest.mark.parametrize("case", SOLVE_BAD, ids=[c[0] for c in SOLVE_BAD])
def test_solve_yaw_refusals_of_its_own(lib, case):
    _, kw, word = case
    assert _solve_yaw(lib, **kw) == capi.ERR_ARG and word in err_of(lib), err_of(lib)


def test_solve_yaw_accepted_values_reach_the_solver_check(lib):
    for kw in (dict(normal_up=1.0), dict(normal_up=-1.0), dict(up=(0.0, 0.0, 5.0)), dict(size=1), dict(opts=_opts(dict(enable=0)))):
        assert _solve_yaw(lib, **kw) == capi.ERR_ARG and "solver is null" in err_of(lib), err_of(lib)


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_basis_at_the_level_camera_reproduces_r_front():
    u = (0.0, -1.0, 0.0)
    h1, h2 = Y.basis(u)
    assert h1 == (0.0, 0.0, 1.0) and h2 == (-1.0, 0.0, 0.0)
    R, cs, sn = Y.rotation(0.0, u, h1, h2, 0.0, Y.tilt_c(0.0))
    assert (cs, sn) == (1.0, 0.0) and np.array_equal(np.array(R), P.R_FRONT)


def test_no_basis_along_gravity_and_at_a_flat_plate():
    assert Y.basis((0.0, 0.0, 1.0)) is None and Y.basis((0.0, 0.0, -1.0)) is None
    a = math.radians(0.5)                                       # |g|^2 = sin^2 = 7.6e-5 < 1e-4
    assert Y.basis((0.0, -math.sin(a), -math.cos(a))) is None and Y.basis((0.0, -math.sin(2 * a), -math.cos(2 * a))) is not None
    assert Y.basis((math.nan, 0.0, 0.0)) is None
    assert Y.tilt_c(1.0) == 0.0 and Y.tilt_c(-1.0) == 0.0 and Y.tilt_c(0.0) == 1.0
    quad = L.lean_back_set()[0]
    assert Y.solve(YS.CAM, quad["pts"], 0, (0.0, 0.0, 1.0), L.S)["state"] == -1
    assert Y.solve(YS.CAM, quad["pts"], 0, quad["u"], 1.0)["state"] == -1
    bad = quad["pts"].copy(); bad[2, 1] = np.nan
    assert Y.solve(YS.CAM, bad, 0, quad["u"], L.S)["state"] == 0
    r = Y.solve(YS.CAM, quad["pts"], 0, -quad["u"], L.S, rounds=2)
    assert r["lane"][2:] == [-1] * 4 and (r["state"] == -1 or r["lane"][0] >= 0)


def test_rotation_is_orthonormal_over_a_grid():
    """R(tau)^T R(tau) is the identity to 1e-15 for every u, s, tau of the grid: columns n, y, z are built from unit h1, h2
    and u alone.  Beside that, an addition of this test: det R = 1 and n . u = s, each to 4e-15 -- the determinant is a sum of
    six triple products of entries below one, each with three roundings of 1.1e-16, and n . u a sum of three such products."""
    rng = np.random.default_rng(5)
    worst, worst_det, worst_tilt = 0.0, 0.0, 0.0
    ups = [np.array([0.0, -1.0, 0.0])] + [v / np.linalg.norm(v) for v in rng.normal(size=(12, 3))]
    for u in ups:
        b = Y.basis(u)
        if b is None:
            continue
        for s in (-1.0 + 1e-9, -0.7, L.S, 0.0, 0.3, 0.999):
            for tau in (-4.0, -1.0, -0.31, 0.0, 1e-9, 0.5, 1.0, 3.7):
                R, cs, sn = Y.rotation(tau, tuple(float(v) for v in u), b[0], b[1], s, Y.tilt_c(s))
                R = np.array(R)
                worst = max(worst, np.abs(R.T @ R - np.eye(3)).max())
                worst_det = max(worst_det, abs(np.linalg.det(R) - 1.0))
                worst_tilt = max(worst_tilt, abs(R[:, 0] @ u - s))
    assert worst <= 1e-15, worst
    assert worst_det <= 4e-15 and worst_tilt <= 4e-15, (worst_det, worst_tilt)


def test_a_noise_free_lean_back_pose_is_recovered_to_the_last_step():
    """Exact corners of a plate leaning back 15 degrees: the search's tau is within the last round's grid step of tan(psi / 2)
    of the generating yaw, and the translation is the generating one to 1e-5 of the distance (a step of 1e-6 in tau turns the
    plate by 2e-6 rad).  The walk is given the exact normalised corners in float64: the float32 pixels and the solver's five
    undistortion steps are errors of the points, not of the search.  Every pose of the set that is seen from the front:
    13 of the 400 generating poses show the plate's back (n . t <= 0: a yaw of 45 - 60 degrees towards the side of the frame
    the plate stands on); the model refuses those by definition and reports the nearest admissible yaw there."""
    checked = behind = 0
    for c in L.lean_back_set():
        if not c["R"][:, 0] @ c["t"] > 0.0:
            behind += 1
            continue
        X = (c["R"] @ P.object_points(L.SIZE).T).T + c["t"]
        nxy = (X[:, :2] / X[:, 2:]).reshape(8)
        r = Y.solve(YS.CAM, None, L.SIZE, c["u"], L.S, nxy=nxy)
        assert r["state"] == 1
        want = math.tan(math.radians(Y.yaw_of(c["R"], c["u"])) / 2)
        assert abs(r["tau"] - want) <= r["step"], (r["tau"], want, r["step"])
        assert np.abs(r["t"] - c["t"]).max() <= 1e-5 * np.linalg.norm(c["t"])
        assert 0 < r["step"] <= (2.0 / 63) ** 4 * 1.0001
        checked += 1
    assert checked == L.N_POSES - behind and behind == 13


def test_rounds_converge():
    """Four rounds agree with six to the fourth round's step on the whole set."""
    worst = 0.0
    for c, r4 in zip(L.lean_back_set()[::8], YS.reference_set()[::8]):
        r6 = Y.solve(YS.CAM, c["pts"], L.SIZE, c["u"], L.S, rounds=6)
        assert r6["lane"][:4] == r4["lane"][:4]
        worst = max(worst, abs(r6["tau"] - r4["tau"]))
    assert worst <= (2.0 / 63) ** 4 * 1.0001


# ---- the statistics of DESIGN.md section 27 -----------------------------------------------------------------------------
@pytest.mark.parametrize("tilt", [0.0, 2.0], ids=["true-up", "up-off-by-2deg"])
def test_yaw_error_counts_on_the_lean_back_set(tilt, capsys):
    e_min, e_pri, e_yaw = YS.set_errors(tilt)
    s_min, s_pri, s_yaw = YS.stats(e_min), YS.stats(e_pri), YS.stats(e_yaw)
    with capsys.disabled():
        print(f"\n[yaw solve] up off by {tilt} deg: min-error {s_min}\n[yaw solve] prior {s_pri}\n[yaw solve] constrained {s_yaw}")
    assert len(e_yaw) == L.N_POSES and all(r["state"] == 1 for r in YS.reference_set(tilt))
    assert s_yaw["over10"] < s_pri["over10"] < s_min["over10"]
