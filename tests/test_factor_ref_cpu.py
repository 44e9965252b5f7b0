"""The extended-precision factor reference (tests/factor_ref.py) and its cases (tests/factor_cases.py), checked on the CPU:

  * every named case provably has the property it is named for;
  * the reference reproduces closed forms (constant acceleration, constant rate about one axis, zero baseline, the round trip of Plus);
  * its two claims about upstream's Jacobians hold on every case: all blocks are derivatives except the IMU factor's first-order rotation rows,
    which are derivatives exactly where Bg_i equals the linearisation point;
  * the oracle, a plain float64 restatement, stays inside the bounds the GPU test (tests/test_gpu_factor_edges.py) applies to the device: 64 eps
    scale for the short sums; for the recursions and factorisations its error is that test's yardstick, and is checked here only against a
    ceiling of 16 n eps scale (n steps, each a product with an F of at most 15 terms per entry) so that a broken reference or oracle shows.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

import factor_cases as fc
import factor_ref as fr

SHORT = 64.0
IMU = sorted(fc.imu_cases())
PROJ = sorted(fc.proj_cases())


def test_constants_mirror_the_default_configuration(P):
    cfg = P.default_config()
    assert (cfg.g_norm, cfg.height, cfg.width, cfg.focal_length, cfg.depth_max) == (fc.G_NORM, fc.HEIGHT, fc.WIDTH, fc.FOCAL, fc.DEPTH_MAX)
    assert (cfg.acc_n, cfg.gyr_n, cfg.acc_w, cfg.gyr_w) == tuple(fc.NOISE[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w"))
    assert np.array_equal(np.array(cfg.tic[:]), fc.TIC) and np.array_equal(np.array(cfg.ric[:]).reshape(3, 3), fc.RIC)


def test_imu_cases_have_their_properties():
    cs = fc.imu_cases()
    assert [cs["n%d" % n]["n"] for n in (1, 7, 8, 9, 17, 64, 65, 400)] == [1, 7, 8, 9, 17, 64, 65, 400] and (fc.PI_CH, fc.SLOT_CAP) == (8, 64)
    assert cs["n400"]["longdouble"] and not any(c["longdouble"] for k, c in cs.items() if k != "n400")
    assert all(len(c["dt"]) == c["n"] and c["acc"].shape == (c["n"], 3) and c["gyr"].shape == (c["n"], 3) for c in cs.values())
    d = cs["dt_spread"]["dt"]
    assert 1e-4 <= d.min() < 3e-4 and 0.02 < d.max() <= 0.05
    z = cs["dt_zero"]
    assert list(np.where(z["dt"] == 0)[0]) == [4, 8] and z["n"] == 9 and all(np.array_equal(z[k][q], z[k][q - 1]) for k in ("acc", "gyr") for q in (4, 8))
    h = cs["high_dynamics"]
    assert np.abs(h["gyr"]).max() > 12 and np.abs(h["acc"] - [0, 0, 9.8]).max() > 45
    s = cs["standstill"]
    assert np.all(s["acc"] == [0, 0, fc.G_NORM]) and not s["gyr"].any() and np.array_equal(s["pi"], s["pj"]) and not s["sbi"].any() and not s["sbj"].any()
    assert cs["benign"]["pi"][6] > 0 and cs["benign"]["pj"][6] > 0
    assert cs["qw_neg_i"]["pi"][6] < 0 < cs["qw_neg_i"]["pj"][6] and cs["qw_neg_j"]["pj"][6] < 0 < cs["qw_neg_j"]["pi"][6]
    assert cs["qw_neg_both"]["pi"][6] < 0 and cs["qw_neg_both"]["pj"][6] < 0
    b = cs["bias_far"]
    assert abs(np.linalg.norm(b["sbi"][3:6] - b["ba"]) - 0.5) < 1e-12 and abs(np.linalg.norm(b["sbi"][6:9] - b["bg"]) - 0.2) < 1e-12
    assert cs["noise_illcond"]["noise"] == (1.0, 0.01, 1e-6, 1e-6) and len(set(cs["noise_equal"]["noise"])) == 1
    for k, c in cs.items():
        assert c["dbg0"] == k.endswith("_dbg0") or k == "standstill"
        if c["dbg0"]:
            assert np.array_equal(c["sbi"][6:9], c["bg"])
    # the rotation residual of rot_near_pi is within a degree of its largest: |2 vec| = 2 sin(angle / 2)
    c = cs["rot_near_pi"]
    r, _ = fr.imu_residual(fc.imu_preint_ref("rot_near_pi"), fc.G_NORM, c["pi"], c["sbi"], c["pj"], c["sbj"])
    ang = 2 * np.degrees(np.arcsin(min(1.0, np.linalg.norm(r[3:6]) / 2)))
    assert 179.0 < ang < 180.0, ang
    # the covariance of noise_illcond is ill-conditioned, that of one step singular (position rows = dt / 2 x velocity rows: V03 = dt / 2 V63 ...)
    assert np.linalg.cond(fc.imu_preint_ref("noise_illcond")["cov"]) > 1e11 > 1e6 > np.linalg.cond(fc.imu_preint_ref("benign")["cov"])
    one = fc.imu_preint_ref("n1")["cov"]
    assert np.abs(one[0:3] - 0.0025 * one[6:9]).max() <= 1e-15 * np.abs(one[0:3]).max()


def test_projection_cases_have_their_properties(P):
    cs = fc.proj_cases()
    assert sorted({c["cfg_kw"]["tr"] for k, c in cs.items() if k.startswith("tr")}) == [0.0, 0.01, 0.033]
    assert sorted({c["oi"][4] for k, c in cs.items() if k.startswith("tr")}) == [0.0, 240.0, 479.0]
    for k, c in cs.items():
        if k.startswith("tr"):
            assert c["oi"][7] != c["td"] != c["oj"][7] and np.abs(np.r_[c["oi"][5:7], c["oj"][5:7]]).max() == 2.0
    assert (cs["invdep_ub"]["inv_dep"], cs["invdep_1e-3"]["inv_dep"], cs["invdep_10"]["inv_dep"]) == (2.0 / P.default_config().depth_max, 1e-3, 10.0)
    K = (fc.FOCAL, fc.HEIGHT, 0.01)
    for k, dep in (("depj_0.05", 0.05), ("depj_0.2", 0.2), ("depj_neg", -0.7)):
        c = cs[k]
        assert abs(fr.proj_dep_j(K, c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], 0) - dep) < 1e-12
    z = cs["zero_baseline"]
    assert np.array_equal(z["pi"], z["pj"])
    assert cs["qw_neg_i"]["pi"][6] < 0 and cs["qw_neg_j"]["pj"][6] < 0 and cs["qw_neg_ic"]["ex"][6] < 0 < cs["ex_default"]["ex"][6]
    c = cs["rot179"]
    d = fc.qmul(fc.qconj(c["pi"][3:]), c["pj"][3:])
    assert abs(2 * np.degrees(np.arctan2(np.linalg.norm(d[:3]), d[3])) - 179.0) < 1e-9
    assert fr.proj_dep_j(K, c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], 0) > 0.5
    assert np.abs(cs["far_origin"]["pi"][:3]).min() > 9e3 and np.abs(cs["far_origin"]["pj"][:3]).min() > 9e3
    assert np.array_equal(cs["ex_identity"]["ex"], [0, 0, 0, 0, 0, 0, 1])
    for k, lo, hi in (("cauchy_r0", 0.0, 1e-10), ("cauchy_r1", 0.999, 1.001), ("cauchy_r300", 300.0, 320.0)):
        c = cs[k]
        r, _ = fr.proj_residual(K, c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], 0)
        assert lo <= np.linalg.norm(r) <= hi, (k, r)


def test_pose_cases_have_their_properties():
    names, x, d = fc.plus_cases()
    i = names.index
    assert not d[i("d_zero")].any() and abs(np.linalg.norm(d[i("d_1e-20")]) - 1e-20) < 1e-30 and abs(np.linalg.norm(d[i("rot_norm3")][3:]) - 3) < 1e-15
    assert x[i("qw_neg")][6] < 0
    names, x, x0, flip = fc.delta_cases()
    w = [fr.pose_delta(a, b)[2] for a, b in zip(x, x0)]
    i = names.index
    assert np.array_equal(x[i("x_eq_x0")], x0[i("x_eq_x0")]) and w[i("w_exactly_0")] == 0 and -1e-8 < w[i("w_slightly_neg")] < 0 < w[i("w_slightly_pos")] < 1e-8
    assert [not (v >= 0) for v in w] == flip


# ------------------------------------------------------------------------------------------------ closed forms
def test_reference_preintegration_closed_forms():
    n, dt = 50, 0.005
    z3, T = np.zeros(3), n * 0.005
    noise = tuple(fc.NOISE[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w"))
    a = np.array([0.3, -0.2, 9.7])                      # constant acceleration, no rotation: dv = a t, dp = a t^2 / 2
    for ld in (False, True):
        r = fr.preint(np.full(n, dt), np.tile(a, (n, 1)), np.zeros((n, 3)), a, z3, z3, z3, noise, longdouble=ld)
        with mpmath.workdps(40):
            Tm = sum(mpmath.mpf(dt) for _ in range(n))
            assert np.array_equal(r["dv"], [float(mpmath.mpf(x) * Tm) for x in a]) and np.array_equal(r["dp"], [float(mpmath.mpf(x) * Tm * Tm / 2) for x in a])
        assert np.array_equal(r["dq"], [1, 0, 0, 0]) and r["sum_dt"] == float(Tm)
        assert np.array_equal(r["jac"][9:, 9:], np.eye(6)) and np.array_equal(r["jac"][0:3, 0:3], np.eye(3)) and np.array_equal(r["jac"][6:9, 6:9], np.eye(3))
        assert np.array_equal(r["jac"][0:3, 6:9], float(Tm) * np.eye(3)) and not r["jac"][3:6, 0:3].any()
        assert np.allclose(np.diag(r["cov"])[9:12], n * dt ** 2 * noise[2] ** 2, rtol=1e-15) and np.allclose(np.diag(r["cov"])[12:], n * dt ** 2 * noise[3] ** 2, rtol=1e-15)
    w = np.array([0.0, 0.0, 0.5])                       # constant rate about z: every step turns by 2 atan(w dt / 2) (normalised deltaQ)
    r = fr.preint(np.full(n, dt), np.zeros((n, 3)), np.tile(w, (n, 1)), z3, w, z3, z3, noise)
    with mpmath.workdps(40):
        half = n * mpmath.atan(mpmath.mpf(0.5) * mpmath.mpf(dt) / 2)
        assert np.array_equal(r["dq"], [float(mpmath.cos(half)), 0.0, 0.0, float(mpmath.sin(half))])
    assert not r["dp"].any() and not r["dv"].any()
    assert abs(2 * np.arctan2(r["dq"][3], r["dq"][0]) - 0.5 * T) < n * (0.5 * dt) ** 3 / 12 * 1.01


def test_reference_world_state_closed_form():
    """process_imu at constant acceleration and zero rotation: deltaQ(0) is the identity, so R stays as given bit for bit, the world acceleration
    A = R (a - Ba) - g is constant, and the midpoint recursion sums to V0 + A T and P0 + V0 T + A T^2 / 2 for any partition of T into steps."""
    rng = np.random.default_rng(3)
    n = 37
    dt = rng.uniform(1e-3, 2e-2, n)
    a, Ba, g = np.array([0.3, -0.2, 9.7]), np.array([0.02, -0.01, 0.03]), np.array([0.0, 0.0, 9.805])
    P0, V0, z3 = np.array([1.5, -2.0, 0.7]), np.array([0.4, 0.1, -0.3]), np.zeros(3)
    q = fc.axis_angle([0.3, -0.5, 0.8], 40.0)
    R0 = np.array([[float(x) for x in r] for r in fr.q2R((q[3], q[0], q[1], q[2]))])
    r = fr.process_imu(dt, np.tile(a, (n, 1)), np.zeros((n, 3)), a, z3, P0, R0, V0, Ba, z3, g)
    assert np.array_equal(r["R"], R0)
    with mpmath.workdps(40):
        m = lambda v: [mpmath.mpf(float(x)) for x in v]
        T = sum(m(dt))
        A = fr.sub(fr.mv([m(row) for row in R0], fr.sub(m(a), m(Ba))), m(g))
        V = [v0 + x * T for v0, x in zip(m(V0), A)]
        Pm = [p0 + v0 * T + x * T * T / 2 for p0, v0, x in zip(m(P0), m(V0), A)]
        assert np.array_equal(r["V"], [float(x) for x in V]) and np.array_equal(r["P"], [float(x) for x in Pm])
    assert r["scale_p"] >= np.abs(r["P"]).max() and r["scale_v"] >= np.abs(r["V"]).max() and r["scale_r"] >= np.abs(R0).max() * 0.999


def test_reference_zero_baseline_and_round_trip():
    c = fc.proj_cases()["zero_baseline"]
    for use_td in (0, 1):
        K = (fc.FOCAL, fc.HEIGHT, c["cfg_kw"]["tr"])
        a = (c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], use_td)
        r, rs = fr.proj_residual(K, *a)
        ti = c["td"] - c["oi"][7] + K[2] / K[1] * (c["oi"][4] - K[1] / 2)
        tj = c["td"] - c["oj"][7] + K[2] / K[1] * (c["oj"][4] - K[1] / 2)
        pi_, pj_ = c["oi"][:2] - use_td * ti * c["oi"][5:7], c["oj"][:2] - use_td * tj * c["oj"][5:7]
        # identical float64 poses; the quaternions are unit only to round-off and Eigen's q * v does not normalise: a few eps of the scale remain
        assert fr.ratio(r, fc.FOCAL / 1.5 * (pi_ - pj_), rs).max() <= 8
        J = fr.proj_jacobian_derivative(K, *a)
        _, Js = fr.proj_jacobian_formula(K, *a)
        assert fr.ratio(J[:, 19], 0.0, Js[:, 19]).max() <= 8 and np.abs(J[:, 19]).max() < 1e-10
    x0 = fc.plus_cases()[1][0]
    for d in fc.ROUND_TRIP_D:                            # rotation part of delta(Plus(x0, d), x0) = d / sqrt(1 + |d|^2 / 4); here Plus is not rounded
        with mpmath.workdps(40):
            num = fr._num("mp")
            x = fr.plus(fr._vec(num, x0), fr._vec(num, d))
            q = fr.qmul(fr.qinv(fr.pose_q(fr._vec(num, x0))), fr.pose_q(x))
            got = np.array([float(2 * v) for v in q[1:]])
        want = d[3:] / np.sqrt(1 + d[3:] @ d[3:] / 4)
        assert np.abs(got - want).max() <= 4 * fr.EPS * np.abs(want).max() + 1e-35


# ------------------------------------------------------------------------------------------------ the oracle on every case
@pytest.mark.parametrize("name", IMU)
def test_oracle_preintegration_and_imu_factor(P, orc, name):
    c = fc.imu_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    ref = fc.imu_preint_ref(name)
    assert ref["source"] == ("longdouble" if c["longdouble"] else "mpmath")
    o = fc.OraclePreint(orc, cfg, c)
    pre461 = o.get()
    assert np.isfinite(pre461).all()
    R = fc.preint_ratios(pre461, ref)
    worst = max(R["dp"], R["dq"], R["dv"], R["sum_dt"], R["jac"].max(), R["cov"].max())
    print("%s: oracle pre-integration dp %.2f dq %.2f dv %.2f sum_dt %.2f jac %.2f cov %.2f (eps scale)" % (name, R["dp"], R["dq"], R["dv"], R["sum_dt"],
                                                                                                       R["jac"].max(), R["cov"].max()))
    assert worst <= 16 * max(c["n"], 1), R
    # the factor on the oracle's own pre-integration, as float64 values given
    pre = fr.pre_from_461(pre461, c["ba"], c["bg"])
    a = (pre, cfg.g_norm, c["pi"], c["sbi"], c["pj"], c["sbj"])
    r, rs = fr.imu_residual(*a)
    Jf, Js = fr.imu_jacobian_formula(*a)
    Jd = fr.imu_jacobian_derivative(*a)
    ro, Jo = o.raw()
    exact = ~fr.IMU_ZERO & ~fr.IMU_ROT_ROWS
    # upstream's formulas are derivatives in every exact block, and in the rotation rows where Bg_i = bg ...
    assert fr.ratio(Jf, Jd, Js, fr.DIFF_SLACK)[exact].max() <= 8 and not Jd[fr.IMU_ZERO].any() and not Jf[fr.IMU_ZERO].any()
    rot = fr.ratio(Jf, Jd, Js, fr.DIFF_SLACK)[fr.IMU_ROT_ROWS].max()
    if c["dbg0"]:
        assert rot <= 8, rot
    else:   # ... and differ from them by a term of first order in dq_dbg dbg elsewhere
        th = np.linalg.norm(pre["jac"][3:6, 12:15] @ (c["sbi"][6:9] - c["bg"]))
        assert 1e3 < rot and np.abs(Jf - Jd)[fr.IMU_ROT_ROWS].max() <= 4 * th * Js[fr.IMU_ROT_ROWS].max(), (rot, th)
    print("%s: oracle raw residual %.2f, raw Jacobian %.2f (eps scale)" % (name, fr.ratio(ro, r, rs).max(), fr.ratio(Jo, Jf, Js).max()))
    assert fr.ratio(ro, r, rs).max() <= SHORT
    assert fr.ratio(Jo, Jf, Js).max() <= SHORT and not Jo[fr.IMU_ZERO].any()
    assert fr.ratio(Jo, Jd, Js, fr.DIFF_SLACK)[exact | (fr.IMU_ROT_ROWS & c["dbg0"])].max() <= SHORT
    if name == "standstill":
        assert np.abs(r).max() <= SHORT * fr.EPS * rs.max() and np.abs(ro).max() <= SHORT * fr.EPS * rs.max()
    # whitening: LLT(cov^-1) against cov, and the Gram matrix the solver consumes
    wh = fr.whiten_identity_error(o.sqrt_info(), pre["cov"]) / fr.EPS
    rw, Jw = o.whitened()
    A = np.hstack([Jw, rw[:, None]])
    gr = fc.gram_scaled_error(A.T @ A, fr.gram_ref(Jo, ro, pre["cov"]))
    print("%s: oracle whitening |S cov S^T - I| %.3g eps, Gram %.3g eps (cond %.2g)" % (name, wh, gr, np.linalg.cond(pre["cov"])))
    # these two are the GPU test's yardsticks, not bounded here: after one step the covariance is singular (see the case test) and no whitening exists
    assert np.isfinite([wh, gr]).all()
    o.close()


def test_oracle_duplicated_stamp_leaves_jacobian_and_covariance(P, orc):
    """The step of a duplicated stamp (dt = 0) is the identity on everything but the re-normalised delta_q: F = I and V = 0 exactly."""
    c = fc.imu_cases()["dt_zero"]
    cfg = P.default_config()
    a = fc.OraclePreint(orc, cfg, c).get()
    c2 = fc.without_last(c)
    b = fc.OraclePreint(orc, cfg, c2).get()
    assert fc.same_but_dq(a, b) and np.isfinite(a).all()
    r = fr.preint(c2["dt"], c2["acc"], c2["gyr"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"])
    ref = fc.imu_preint_ref("dt_zero")
    assert fc.same_but_dq(fr.pre_to_461(r), fr.pre_to_461(ref))


@pytest.mark.parametrize("name", PROJ)
def test_oracle_projection_factor(P, orc, name):
    c = fc.proj_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    K = fr.proj_consts(cfg)
    for use_td in (0, 1):
        a = (c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], use_td)
        r, rs = fr.proj_residual(K, *a)
        Jf, Js = fr.proj_jacobian_formula(K, *a)
        Jd = fr.proj_jacobian_derivative(K, *a)
        ro, Jo = fc.oracle_projection(orc, cfg, c, use_td)
        e = (fr.ratio(Jf, Jd, Js, fr.DIFF_SLACK).max(), fr.ratio(ro, r, rs).max(), fr.ratio(Jo, Jd, Js, fr.DIFF_SLACK).max())
        print("%s td%d: formula vs derivative %.2f, oracle residual %.2f, oracle Jacobian %.2f (eps scale)" % ((name, use_td) + e))
        assert e[0] <= 8          # every projection column of upstream is a derivative
        assert e[1] <= SHORT and e[2] <= SHORT
        if not use_td:
            assert not Jd[:, 18].any() and not Jf[:, 18].any()


def test_oracle_pose_operations(orc):
    names, x, d = fc.plus_cases()
    po, dxo = np.zeros_like(x), np.zeros((len(x), 6))
    orc.ovio_pose_ops(len(x), x.ctypes.data, d.ctypes.data, x.ctypes.data, po.ctypes.data, dxo.ctypes.data)
    for i, n in enumerate(names):
        v, s = fr.pose_plus(x[i], d[i])
        assert fr.ratio(po[i], v, s).max() <= SHORT, n
        assert abs(np.linalg.norm(po[i][3:]) - 1) <= 4 * fr.EPS
    names, x, x0, flip = fc.delta_cases()
    po, dxo, z = np.zeros_like(x), np.zeros((len(x), 6)), np.zeros((len(x), 6))
    orc.ovio_pose_ops(len(x), x.ctypes.data, z.ctypes.data, x0.ctypes.data, po.ctypes.data, dxo.ctypes.data)
    for i, n in enumerate(names):
        v, s, w = fr.pose_delta(x[i], x0[i])
        assert fr.ratio(dxo[i], v, s).max() <= SHORT, n
    i = names.index
    assert np.array_equal(dxo[i("w_exactly_0")][3:], [2, 0, 0]) and dxo[i("w_slightly_neg")][3] < -1.9 and dxo[i("w_slightly_pos")][3] > 1.9
    assert not dxo[i("x_eq_x0")][:3].any() and np.abs(dxo[i("x_eq_x0")][3:]).max() <= SHORT * fr.EPS
