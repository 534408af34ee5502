"""The independent IPPE reference (tests/pnp_ref.py) on the pose zoo: it recovers the generating pose where the contract's
undistortion has converged, the CPU oracle agrees with it over the whole zoo (rotations as MATRICES: at theta = pi, rvec
and -rvec are one rotation), and the comparison sees four deliberately wrong solvers.  Runs without a GPU."""
import collections

import numpy as np

import pnp_ref as P
from oracle import oracle


def _named(idx, Z, extra=None, n=6):
    return [(Z[i]["name"],) + ((extra[i],) if extra is not None else ()) for i in idx[:n]]


def test_zoo_shares_and_conditions():
    """Conditions on the zoo, from the two reference runs alone: few ill-conditioned poses, few ambiguous ones outside the
    deliberately fronto-parallel groups, and every branch the solvers have is reached by some pose."""
    Z = P.zoo()
    r64, rmp, cls = P.zoo_reference()
    print("zoo:", len(Z), "cases;", dict(collections.Counter(c["group"] for c in Z)))
    assert len(Z) >= 1500
    live = [i for i in range(len(Z)) if not cls[i]["degenerate"]]
    ill = [i for i in live if cls[i]["ill"]]
    amb = [i for i in live if cls[i]["ambiguous"]]
    amb_out = [i for i in amb if Z[i]["group"] not in P.FRONTO_GROUPS]
    n_out = sum(Z[i]["group"] not in P.FRONTO_GROUPS for i in live)
    conv = [i for i in live if P.undistortion_converged(Z[i])]
    e64 = np.array([cls[i]["err64"] for i in live])
    print(f"degenerate {len(Z) - len(live)}; ill-conditioned {len(ill)} ({len(ill) / len(Z):.2%}); ambiguous {len(amb)}, outside the "
          f"fronto-parallel groups {len(amb_out)} ({len(amb_out) / n_out:.2%}); undistortion converged in 5 steps {len(conv)} ({len(conv) / len(live):.2%})")
    print(f"float64 vs mpmath reference: median {np.median(e64):.2e}, p99 {np.percentile(e64, 99):.2e}, max {e64.max():.2e}")
    assert len(ill) <= 0.02 * len(Z), _named(ill, Z)
    assert len(amb_out) <= 0.02 * n_out, _named(amb_out, Z)
    # branches, counted from the reference's rotation
    quat = collections.Counter(P.quat_branch(rmp[i]["R"][0]) for i in live)
    gaps = np.array([P.pi_gap(rmp[i]["R"][0]) for i in live])
    ladder = {e: int((gaps < e).sum()) for e in (1e-3, 1e-5, 1e-7, 1e-8)}
    flags = collections.Counter(f for c in Z for f in P.degenerate_flags(*P.CAMERAS[c["cam"]][1:], c["pts"], c["size"]))
    print("rot_to_quat branches:", dict(quat), "; poses with pi - theta below:", ladder, "; degenerate flags:", dict(flags))
    assert all(quat[b] >= 1 for b in ("trace", "x", "y", "z")), quat
    assert ladder[1e-3] >= 1 and ladder[1e-7] >= 1, ladder          # the near-pi branch of rot_to_rvec, deep inside its band
    # `den`, `h8` and `t0` (R_v = identity): reached with exact zeros on the power-of-two camera.  `bdet` and `g2` cannot be reached with finite
    # float32 pixels: det B = sqrt(p^2 + q^2 + 1) > 0 for every finite (p, q), and g2 = 0 needs J = 0, i.e. a rank-1
    # homography, which den != 0 excludes; only a NaN raises them, and non-finite values go through irmv_pnp_solve alone.
    assert flags["den"] >= 1 and flags["h8"] >= 1 and flags["t0"] >= 1, flags


def test_reference_recovers_the_generating_pose():
    """Where 5 and 50 undistortion steps agree to 1e-9, the pixels carry no noise and the two solutions' errors are apart, the
    mpmath reference returns the pose the quad was projected from.  What is left is the float32 rounding of the pixels:
    delta <= 2^-24 |pixel| over a quad whose smaller image extent is h px, eps = delta / h; an in-plane angle moves by ~ eps,
    the tilt phi read from the foreshortening cos(phi) by eps / sin(phi), at worst sqrt(2 eps) -> |dR| <= 4 sqrt(eps);
    the plate centre moves by ~ dist * eps along the ray and dist * delta / f across it -> |dt| <= 8 dist eps."""
    Z = P.zoo()
    r64, rmp, cls = P.zoo_reference()
    tested, worst_R, worst_t = 0, 0.0, 0.0
    posed = [i for i in range(len(Z)) if Z[i]["R"] is not None and Z[i]["noise"] == 0]
    for i in posed:
        c = Z[i]
        if cls[i]["degenerate"] or cls[i]["ambiguous"] or not P.undistortion_converged(c):
            continue
        ext = np.ptp(c["pts"].astype(np.float64), axis=0)
        sides = np.linalg.norm(np.diff(np.vstack([c["pts"], c["pts"][:1]]).astype(np.float64), axis=0), axis=1)
        eps = 2.0 ** -24 * max(np.abs(c["pts"]).max(), 1.0) / max(min(sides.min(), ext.max()), 1e-3)
        dist = np.linalg.norm(c["t"])
        eR, et = np.abs(rmp[i]["R"][0] - c["R"]).max(), np.abs(rmp[i]["t"][0] - c["t"]).max()
        tested += 1
        worst_R, worst_t = max(worst_R, eR / (4 * np.sqrt(eps))), max(worst_t, et / (8 * dist * eps + 1e-9))
        assert eR <= 4 * np.sqrt(eps) and et <= 8 * dist * eps + 1e-9, (c["name"], eR, et, eps)
    print(f"true pose recovered on {tested} of {len(posed)} noise-free posed cases ({tested / len(Z):.1%} of the zoo); "
          f"worst error / bound: R {worst_R:.3f}, t {worst_t:.3f}")
    assert tested >= 300


def _compare_all(solve):
    """solve(case) -> (R, t, ok): the indices of the zoo cases on which it fails the comparison."""
    Z = P.zoo()
    _, rmp, cls = P.zoo_reference()
    bad = []
    for i, c in enumerate(Z):
        R, t, ok = solve(c)
        if not P.check(R, t, ok, rmp[i], cls[i])[0]:
            bad.append(i)
    return bad


def _oracle_solve(c):
    _, K, D = P.CAMERAS[c["cam"]]
    o = oracle.solve_pnp_ippe(K, D, c["pts"], c["size"])
    return P.matrix_of(o["rvec"]), o["tvec"], o["ok"]


def test_oracle_matches_reference_over_the_zoo():
    """The oracle's closed-form derivation against the independent one, every case of the zoo: the rotation its rvec ENCODES
    and tvec within the pose's bar (1e-6; ill-conditioned: 10 x the float64 reference's own error), `ok` identical; rvec itself
    where pi - theta > 1e-3, up to the choice among the two solutions of an ambiguous pose.
    Before rot_to_rvec took the axis from the symmetric part near pi, this failed on pi-roll-centred5-s0-d0.8-eps{0,1e-09,1e-11}
    (pi - theta = 9.3e-8 after the pixels' float32 rounding): 2.8e-6 in the rotation."""
    Z = P.zoo()
    _, rmp, cls = P.zoo_reference()
    bad = _compare_all(_oracle_solve)
    assert not bad, _named(bad, Z)
    worst, n_rvec, worst_rvec = 0.0, 0, 0.0
    for i, c in enumerate(Z):
        if cls[i]["degenerate"]:
            continue
        _, K, D = P.CAMERAS[c["cam"]]
        o = oracle.solve_pnp_ippe(K, D, c["pts"], c["size"])
        assert o["ok"] == rmp[i]["ok"], c["name"]
        _, err, which = P.check(P.matrix_of(o["rvec"]), o["tvec"], o["ok"], rmp[i], cls[i])
        if not cls[i]["ill"]:
            worst = max(worst, err)
        if P.pi_gap(rmp[i]["R"][which]) > 1e-3 and not cls[i]["ill"]:
            n_rvec += 1
            d = np.abs(o["rvec"] - P.rvec_of(rmp[i]["R"][which])).max()
            worst_rvec = max(worst_rvec, d)
            assert d <= P.BAR, (c["name"], d)
    print(f"oracle vs mpmath reference: worst error on well-conditioned poses {worst:.2e}; rvec compared on {n_rvec} poses, worst {worst_rvec:.2e}")


def test_near_pi_rvec_is_well_conditioned():
    """The pi - eps ladder: the rotation the oracle's rvec encodes meets the plain 1e-6 bar on every rung."""
    Z = P.zoo()
    _, rmp, cls = P.zoo_reference()
    n = 0
    for i, c in enumerate(Z):
        if c["group"] not in ("pi_roll", "pi_axis") or cls[i]["degenerate"]:
            continue
        assert not cls[i]["ill"], c["name"]
        R, t, ok = _oracle_solve(c)
        passed, err, _ = P.check(R, t, ok, rmp[i], cls[i])
        assert passed and err <= P.BAR, (c["name"], err)
        n += 1
    assert n >= 200


def test_rot_to_rvec_on_the_pi_ladder_at_matrix_level():
    """The float32 pixels dither the angle a solved pose realises, so the deepest rungs are fed to the oracle's rot_to_rvec
    directly: R = exp((pi - eps) [n]) plus 1e-13 of rounding-sized noise, seeded axes, eps down the ladder.  The rotation the
    rvec encodes stays within 1e-9 of R at every rung (the axis from the antisymmetric part alone is off by 1e-4 at eps = 1e-9);
    rvec itself within 1e-9 where eps >= 1e-3."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for eps in P.PI_LADDER + (1e-2, 0.5, 2.0, np.pi - 1e-6, np.pi - 1e-12):
        for k in range(40):
            n = rng.standard_normal(3) if k >= 6 else np.eye(3)[k % 3] * (1 if k < 3 else -1)
            n = n / np.linalg.norm(n)
            r = n * (np.pi - eps)
            R = P.matrix_of(r) + 1e-13 * rng.standard_normal((3, 3))
            got = oracle.rot_to_rvec(R)
            d = np.abs(P.matrix_of(got) - R).max()
            worst = max(worst, d)
            assert d <= 1e-9, (eps, n, d)
            if eps >= 1e-3:
                assert np.abs(got - r).max() <= 1e-9, (eps, n)
    print(f"rot_to_rvec at matrix level: worst |R(rvec) - R| {worst:.2e}")


def test_out_of_range_coordinates_are_refused():
    """Non-finite coordinates and float32 coordinates that no longer resolve a pixel (|v| >= 2^24; 1e30 overflows nothing in
    fp64 and would come back as a finite, meaningless pose): ok = 0 in the oracle and in both reference runs; the last
    float32 below the limit is still solved."""
    c = next(c for c in P.zoo() if c["group"] == "random" and c["cam"] == 1)
    _, K, D = P.CAMERAS[1]
    for k in range(8):
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, P.PIXEL_LIMIT, -P.PIXEL_LIMIT):
            pts = c["pts"].copy().reshape(8)
            pts[k] = v
            assert not oracle.solve_pnp_ippe(K, D, pts, c["size"])["ok"], (k, v)
            assert not P.solve64(K, D, pts, c["size"])["ok"] and not P.solve_mp(K, D, pts, c["size"])["ok"], (k, v)
        pts = c["pts"].copy().reshape(8)
        pts[k] = np.float32(P.PIXEL_LIMIT - 1)
        a = P.solve64(K, D, pts, c["size"])
        assert a["ok"] and oracle.solve_pnp_ippe(K, D, pts, c["size"])["ok"] and P.solve_mp(K, D, pts, c["size"], hnull=a["hnull"])["ok"], k


def _variant(**kw):
    def solve(c):
        _, K, D = P.CAMERAS[c["cam"]]
        r = P.solve64(K, D, c["pts"], c["size"], **kw)
        return r["R"][0], r["t"][0], r["ok"]
    return solve


def test_comparison_sees_wrong_solvers():
    """The float64 reference itself passes everywhere; each wrong variant of it fails on at least a stated number of poses:
      4 undistortion steps   wherever the 4th -> 5th step still moves a point by > 1e-6: distorting cameras off the principal
                             point, i.e. most of 2/3 of the zoo x 8/9 of the positions; stated: >= 300
      sign rule dropped      (both last-row entries taken non-negative) wrong whenever the two columns' scalar product asks
                             for opposite signs: about half of the tilted poses; stated: >= 300
      half-widths swapped    (small <-> large plate) every well-posed pose: the range scales by 5/3; stated: >= 1400
      second solution        every pose that is not ambiguous; stated: >= 1000"""
    Z = P.zoo()
    assert not _compare_all(_variant())
    for kw, least in ((dict(steps=4), 300), (dict(sign_rule=False), 300), (dict(swap_sizes=True), 1400), (dict(pick_second=True), 1000)):
        bad = _compare_all(_variant(**kw))
        print(f"wrong solver {kw}: caught on {len(bad)} of {len(Z)} poses (stated minimum {least})")
        assert len(bad) >= least, kw
