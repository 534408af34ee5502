"""The pose uncertainty without a GPU (include/irmv_hip.h, "pose uncertainty"): the ABI structs and exports, every refusal the
library makes before it touches the GPU, and irmv_detection_amd.pose_cov (the host reference of the model) against checks
that do not share its code: central differences of its own projection, the product Sigma . A, the scatter of the project's
fp64 solvers under drawn corner noise, and each refusal rule.

Measured on the sets of tests/pose_cov_set.py (figures: DESIGN.md section 31):
  Sigma . A - I, largest entry over hard_set(), both blocks               2.2e-9   (asserted: 100 x)
  |J - J_fd(h)| over its Richardson estimate |J_fd(h) - J_fd(2h)| / 3       1.06     (asserted: 10 x, plus the rounding floor)
  second moment of solve64's poses over cov's diagonal, near the axis       0.958 .. 1.071
  ... at a ray 0.43 rad off the axis of the reference camera                 1.248 .. 1.667  (the distortion's own Jacobian,
      which the model leaves out: the sandwich estimate that has it predicts 1.209 .. 1.658, and the maximum-likelihood
      poses of the same draws scatter by 0.918 .. 1.056 of THAT)
  second moment of yaw_solve's (psi, tau) over yaw_cov's diagonal            0.960 .. 1.019
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as P
import pose_cov_set as S
from conftest import ROOT
from irmv_detection_amd import _build, capi, pose_cov as pc, yaw_solve as ys


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return capi.load()


def err_of(lib):
    return lib.irmv_last_error().decode()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("irmv_engine_set_pose_cov", "irmv_engine_get_pose_cov", "irmv_engine_pose_covs", "irmv_pnp_pose_cov")


def test_struct_sizes_layout_and_exports(lib, tmp_path):
    assert C.sizeof(capi.PoseCovOpts) == 16 and C.sizeof(capi.PoseCov) == 288
    mirrored = {name for name, _, _ in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in mirrored, name
    parts = ['printf("%zu %zu %zu %zu %zu", sizeof(irmv_pose_cov_opts), sizeof(irmv_pose_cov), sizeof(irmv_det), sizeof(irmv_pose_alt), sizeof(irmv_yaw_pose));']
    parts += [f'printf(" %zu", offsetof(irmv_pose_cov_opts, {f}));' for f, _ in capi.PoseCovOpts._fields_]
    parts += [f'printf(" %zu", offsetof(irmv_pose_cov, {f}));' for f, _ in capi.PoseCov._fields_]
    src = tmp_path / "pcv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irmv_hip.h"\nint main(void){' + "".join(parts) + "return 0;}\n")
    exe = tmp_path / "pcv"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == ([16, 288, 160, 104, 144] + [getattr(capi.PoseCovOpts, f).offset for f, _ in capi.PoseCovOpts._fields_] +
                   [getattr(capi.PoseCov, f).offset for f, _ in capi.PoseCov._fields_])      # (the other records stay as they are)


def _opts(kw):
    o = capi.pose_cov_opts_struct(kw.get("enable", 1), kw.get("sigma_px", 1.0))
    if "size" in kw:
        o.struct_size = kw["size"]
    return o


BAD_OPTS = [
    ("struct_size", dict(size=12), "struct_size"),
    ("struct_size0", dict(size=0), "struct_size"),
    ("enable2", dict(enable=2), "enable"),
    ("enable-1", dict(enable=-1), "enable"),
    ("sigma0", dict(sigma_px=0.0), "sigma_px"),
    ("sigma-neg", dict(sigma_px=-1.0), "sigma_px"),
    ("sigma>64", dict(sigma_px=64.0000001), "sigma_px"),
    ("sigma-nan", dict(sigma_px=math.nan), "sigma_px"),
    ("sigma-inf", dict(sigma_px=math.inf), "sigma_px"),
]


@pytest.mark.parametrize("case", BAD_OPTS, ids=[c[0] for c in BAD_OPTS])
def test_set_pose_cov_refuses_before_the_gpu(lib, case):
    """Every refusal names its field and comes before the engine is looked at (a null engine here: the GPU is never touched)."""
    _, kw, word = case
    assert lib.irmv_engine_set_pose_cov(None, C.byref(_opts(kw))) == capi.ERR_ARG
    assert word in err_of(lib), err_of(lib)


def test_accepted_opts_reach_the_engine_check(lib):
    for kw in (dict(sigma_px=64.0), dict(sigma_px=1e-6), dict(enable=0)):
        assert lib.irmv_engine_set_pose_cov(None, C.byref(_opts(kw))) == capi.ERR_ARG and "engine is null" in err_of(lib)
    assert lib.irmv_engine_set_pose_cov(None, None) == capi.ERR_ARG and "opts is null" in err_of(lib)
    assert lib.irmv_engine_get_pose_cov(None, None) == capi.ERR_ARG
    n = C.c_int(0)
    assert lib.irmv_engine_pose_covs(None, 0, None, 0, C.byref(n)) == capi.ERR_ARG


def _pnp_cov(lib, pts=True, n=1, size=0, rvec=True, tvec=True, up=None, sigma_px=1.0, out=True):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    q = (C.c_float * 8)(*range(8))
    r, t = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.0, 0.0, 2.0)
    u = None if up is None else (C.c_double * 3)(*up)
    o = (capi.PoseCov * 1)()
    return lib.irmv_pnp_pose_cov(None, C.cast(q, fp) if pts else None, n, size, C.cast(r, dp) if rvec else None,
                                 C.cast(t, dp) if tvec else None, None if u is None else C.cast(u, dp), sigma_px, o if out else None)


PNP_BAD = [
    ("pts", dict(pts=False), "null"), ("rvec", dict(rvec=False), "null"), ("tvec", dict(tvec=False), "null"), ("out", dict(out=False), "null"),
    ("n<0", dict(n=-1), "null"), ("size", dict(size=2), "armor_size"),
    ("sigma0", dict(sigma_px=0.0), "sigma_px"), ("sigma>64", dict(sigma_px=65.0), "sigma_px"), ("sigma-nan", dict(sigma_px=math.nan), "sigma_px"),
    ("up0", dict(up=(0.0, 0.0, 0.0)), "up"), ("up-nan", dict(up=(math.nan, 0.0, 1.0)), "up"), ("up-inf", dict(up=(math.inf, 0.0, 1.0)), "up"),
]


@pytest.mark.parametrize("case", PNP_BAD, ids=[c[0] for c in PNP_BAD])
def test_pnp_pose_cov_refuses_before_the_gpu(lib, case):
    _, kw, word = case
    assert _pnp_cov(lib, **kw) == capi.ERR_ARG and word in err_of(lib), err_of(lib)


def test_pnp_pose_cov_accepted_values_reach_the_solver_check(lib):
    for kw in (dict(), dict(up=(0.0, -3.0, 0.0)), dict(size=1), dict(sigma_px=64.0), dict(n=0)):
        assert _pnp_cov(lib, **kw) == capi.ERR_ARG and "solver is null" in err_of(lib), err_of(lib)


# ---- the model against checks of another kind ---------------------------------------------------------------------------------
def test_the_series_rotation_is_a_rotation_and_agrees_with_scipy():
    """rodrigues() takes sin and cos from its own series: orthonormal to 1e-15 and scipy's matrix to 4e-15 up to 100 rad
    (the reduction by 2 pi loses what 100 / 2 pi ulps lose), 1e-15 on the hard set."""
    assert max(np.abs(S.rotation_of(c["rvec"]) - P.matrix_of(c["rvec"])).max() for c in S.hard_set()) <= 2e-15
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    for th in (0.0, 1e-300, 1e-9, 0.5, 3.1, math.pi, 4.0, 6.2, 2 * math.pi, 7.0, 100.0):
        R = S.rotation_of(axis * th)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 4e-15, th
        assert np.abs(R - P.matrix_of(axis * th)).max() <= 8e-15, th
    assert S.rotation_of((0.0, 0.0, 0.0)).tolist() == np.eye(3).tolist()


H_STEP = 1e-4
# rounding of a central difference: the projection in pixels (< 4e3) carries 2^-53 relative, twice, over 2 h
FD_ROUNDING = 2.0 * 4e3 * 2.0 ** -53 / (2.0 * H_STEP)


def test_analytic_jacobian_against_central_differences(capsys):
    """J of both blocks against central differences of the reference's own projection.  The truncation error of a central
    difference with step h is (h^2 / 6) r''': estimated per case as |J_fd(h) - J_fd(2h)| / 3 (Richardson); the analytic J may
    differ from J_fd(h) by ten times that plus the rounding floor."""
    worst = 0.0
    for c in S.hard_set():
        for up in (None, pc.unit(c["u"])):
            J = S.analytic_jacobian(c, 1.0, up)
            J1, J2 = S.difference_jacobian(c, H_STEP, 1.0, up), S.difference_jacobian(c, 2 * H_STEP, 1.0, up)
            trunc = np.abs(J1 - J2).max() / 3.0
            dev = np.abs(J - J1).max()
            worst = max(worst, dev / (trunc + FD_ROUNDING))
            assert dev <= 10.0 * (trunc + FD_ROUNDING), (c["name"], up is None, dev, trunc, np.abs(J).max())
    with capsys.disabled():
        print(f"\n[pose_cov] worst |J - J_fd| / (truncation estimate + rounding floor) = {worst:.3f}")


INVERSE_MEASURED = 2.2e-9      # the largest entry of Sigma . A - I over hard_set(), both blocks (12 m, oblique)


def test_inverse_times_normal_matrix_is_the_identity(capsys):
    worst = 0.0
    for c in S.hard_set():
        for up, n in ((None, 6), (pc.unit(c["u"]), 4)):
            J = S.analytic_jacobian(c, 1.0, up)
            A = pc.normal_matrix([list(r) for r in J], n)
            inv = pc.cholesky_inverse(A, n)
            assert inv is not None, c["name"]
            e = float(np.abs(pc.full(inv, n) @ pc.full(A, n) - np.eye(n)).max())
            worst = max(worst, e)
            assert e <= 100.0 * INVERSE_MEASURED, (c["name"], n, e)
            assert np.abs(pc.full(A, n) - J.T @ J).max() <= 1e-12 * np.abs(J.T @ J).max()
    with capsys.disabled():
        print(f"\n[pose_cov] worst |Sigma A - I| = {worst:.3e}")
    assert worst >= INVERSE_MEASURED / 100.0      # (the figure above is this set's, not a stale one)


def test_record_fields_follow_from_cov():
    for c in S.hard_set()[::7]:
        r = S.reference(c, 0.8)
        assert r["state"] == 1 and r["yaw_state"] == 1
        M = pc.full(r["cov"])
        d = c["t"] / np.linalg.norm(c["t"])
        assert abs(r["sigma_range"] - math.sqrt(d @ M[3:, 3:] @ d)) <= 1e-12 * r["sigma_range"]
        assert r["sigma_yaw"] == math.sqrt(r["yaw_cov"][0])
        assert np.linalg.eigvalsh(M).min() > 0 and np.linalg.eigvalsh(pc.full(r["yaw_cov"], 4)).min() > 0
        # one pose for both blocks here: one sum of squares (what is left of it is float32 and, at the corners of the strongly
        # distorted camera, the five-step undistortion: up to 6.8 at 0.8 px)
        assert 0.0 <= r["chi2"] == r["yaw_chi2"]
        # sigma_px scales the covariance by its square
        r2 = S.reference(c, 1.6)
        assert np.allclose(np.array(r2["cov"]), 4.0 * np.array(r["cov"]), rtol=1e-9, atol=0)
        # the yaw variance is the rotation block seen along u, constrained: never above the free one
        u = np.array(pc.unit(c["u"]))
        assert r["yaw_cov"][0] <= (u @ M[:3, :3] @ u) * (1 + 1e-9)
        ros = np.array(pc.ros_covariance(r["cov"])).reshape(6, 6)
        assert ros[0, 0] == M[3, 3] and ros[5, 5] == M[2, 2] and ros[0, 3] == M[3, 0] and np.array_equal(ros, ros.T)


def test_the_measured_corners_enter_the_residuals_only():
    """J is taken at the pose and the plate's model: cov is the same bits whatever the measured corners are, chi2 is not."""
    c = S.hard_set()[5]
    a = S.reference(c)
    moved = dict(c, pts=(c["pts"] + np.float32(1.5)).astype(np.float32))
    b = S.reference(moved)
    assert a["cov"] == b["cov"] and a["yaw_cov"] == b["yaw_cov"] and b["chi2"] > 1.0 > a["chi2"]
    pinched = dict(c, pts=c["pts"].copy())
    pinched["pts"][2:4] = pinched["pts"][0:2]          # LT on LB: a coincident pair of MEASURED corners
    assert S.reference(pinched)["cov"] == a["cov"]


# ---- statistical meaning --------------------------------------------------------------------------------------------------
THREE_SIGMA = 3.0 * S.STAT_SAMPLING
IPPE_WORST_NEAR, IPPE_WORST_OFF, YAW_WORST = 1.071, 1.667, 1.019      # measured (the module's docstring)


@pytest.mark.parametrize("k", range(len(S.STAT_POSES)))
def test_cov_is_the_scatter_of_the_fp64_solver(k, capsys):
    """STAT_DRAWS draws of corner noise at STAT_SIGMA_PX, pnp_ref.solve64 on the branch of the noise-free solution.  No
    unbiased estimator scatters by less than (J^T J)^-1 of ITS noise: the lower bound is 1 - 3 sampling errors of the
    distortion-aware prediction.  The upper margin is the measured worst ratio plus one sampling error, per group.  The
    same draws refined to the model's own minimum must scatter by the sandwich estimate, which is where the distortion's
    Jacobian -- the one thing the model leaves out -- is put back."""
    r = S.stat_ippe(k)
    with capsys.disabled():
        print(f"\n[pose_cov] pose {k}: solve64 / cov {np.round(r['ratio'], 3)} range {r['ratio_range']:.3f}  ml / cov {np.round(r['ratio_ml'], 3)}"
              f"  predicted {np.round(r['predicted'], 3)}  ml / sandwich {np.round(r['ratio_sandwich'], 3)}  mirror at {r['separation']:.0f} sigma")
    assert r["separation"] >= S.STAT_SEPARATION                     # the mirror flip is excluded by construction: none of the set
    worst = IPPE_WORST_NEAR if k < S.N_YAW_POSES else IPPE_WORST_OFF
    allr = np.concatenate([r["ratio"], [r["ratio_range"]]])
    assert (allr <= worst + S.STAT_SAMPLING).all(), allr
    assert (r["ratio"] >= r["predicted"] * (1.0 - THREE_SIGMA)).all(), (r["ratio"], r["predicted"])
    assert (np.abs(r["ratio_sandwich"] - 1.0) <= THREE_SIGMA).all(), r["ratio_sandwich"]


@pytest.mark.parametrize("k", range(S.N_YAW_POSES))
def test_yaw_cov_is_the_scatter_of_the_yaw_solver(k, capsys):
    r = S.stat_yaw(k)
    with capsys.disabled():
        print(f"\n[pose_cov] pose {k}: yaw_solve / yaw_cov {np.round(r['ratio'], 3)}  sigma_yaw {math.degrees(r['sigma_yaw']):.3f} deg")
    assert (r["ratio"] <= YAW_WORST + S.STAT_SAMPLING).all() and (r["ratio"] >= 1.0 - THREE_SIGMA).all(), r["ratio"]


def test_the_chosen_set_excludes_nothing():
    assert len(S.STAT_POSES) == 7 and S.N_YAW_POSES == 5
    assert all(S.stat_ippe(k)["separation"] >= S.STAT_SEPARATION for k in range(len(S.STAT_POSES)))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
CAM0 = S.camera(0)
QUAD = np.array([300.0, 330, 300, 270, 420, 270, 420, 330], np.float32)


def _refused(r):
    return S.is_zero_record(r, -1)


def test_a_coincident_corner_pair_of_the_plate_is_rank_deficient(monkeypatch):
    """A plate of height zero (LB on LT, RB on RT) in the camera's y-z plane: no corner moves under a rotation about the
    camera's y axis, that column of J is exactly zero, and the second pivot is exactly 0: refused, by the pivot rule."""
    assert pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 2.0))["state"] == 1
    monkeypatch.setattr(pc, "HALF_Z", (0.0, 0.0))
    J, _ = pc.jacobian(pc.rodrigues((0.0, 0.0, 0.0)), [0.0, 0.0, 2.0], ys.undistort4(CAM0, QUAD), 0, CAM0[0], CAM0[1], 1.0)
    assert all(row[1] == 0.0 for row in J)
    assert pc.cholesky_inverse(pc.normal_matrix(J, 6), 6) is None
    assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 2.0)))
    assert pc.cholesky_inverse([1.0, 1.0, 1.0], 2) is None and pc.cholesky_inverse([1.0, 2.0, 1.0], 2) is None
    assert pc.cholesky_inverse([math.nan, 0.0, 1.0], 2) is None


def test_a_corner_behind_the_camera_is_refused():
    assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.01)))      # the plate spans z = 0.01 +- 0.0275
    assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, -2.0)))
    assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0275)))    # depth exactly 0
    ok = pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), yaw=((0.0, 0.0, 0.0), (0.0, 0.0, -2.0), (0.0, -1.0, 0.0)))
    assert ok["state"] == 1 and ok["yaw_state"] == -1 and not any(ok["yaw_cov"]) and ok["sigma_yaw"] == 0.0 == ok["yaw_chi2"]


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf, 2.0 ** 24])
def test_a_non_finite_input_is_refused(bad):
    for i in (0, 3, 7):
        q = QUAD.copy(); q[i] = bad
        assert _refused(pc.pose_cov(CAM0, q, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 2.0)))
    if bad != 2.0 ** 24:
        for i in range(3):
            v = [0.0, 0.0, 2.0]; v[i] = bad
            assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), v))
            assert _refused(pc.pose_cov(CAM0, QUAD, 0, v, (0.0, 0.0, 2.0)))


def test_a_non_finite_output_is_refused():
    """A plate 1e160 m away: A's entries underflow, the inverse overflows."""
    assert _refused(pc.pose_cov(CAM0, QUAD, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 1e160)))
