"""The factor kernels (csrc/be_factors.h, the propagation routines of csrc/be_preint.h, imu_block_mfma) against their definitions in extended
precision (tests/factor_ref.py) on the named edge cases of tests/factor_cases.py, through stage entries that run each routine alone.

Bounds, none of them taken from the device's output:
  * short sums of products (raw residual, raw Jacobian, projection, pose operations): 64 eps scale, with the reference's cancellation-aware scale per
    entry;
  * recursions and factorisations (pre-integration over n steps, whitening, the Gram matrix): the oracle's own float64 error against the reference on
    the same case is the yardstick; the device may be 4 times that plus 16 eps scale.  Granularity: dp, dq, dv, sum_dt each; every 3 x 3 block of the
    Jacobian (scale: the block's largest reference entry) and of the covariance (entries over sqrt(cov_ii cov_jj)); the whitening identity as a whole;
    the Gram matrix as the largest entry-wise error over sqrt(G_ii G_jj).  For the whitening the oracle is handed the device's covariance, so both
    factor the same matrix (the oracle LLT(cov^-1), the device chol(cov)^-1).
Every case goes through every check.  One case needs a remark, not an exception: after a single step (n1) the covariance is singular in exact
arithmetic (its position rows are dt / 2 times its velocity rows), no whitening exists, the oracle's error is O(1) and the bound is accordingly void;
there the test pins the contract instead: the device and the oracle both report the failed factorisation by an all-zero whitening matrix, and the
Gram block is exactly zero.  In every other case the device's factor has a positive diagonal.

Measured on an MI355X, worst over the cases of a family, device error in units of its bound's scale (and the oracle's where it is the yardstick):
  IMU family      pre-integration dp / dq / dv / jac / cov          raw r   raw J   M cov M^T - I      Gram
                  (device = oracle, bit for bit, in every case)                    device / oracle    device / oracle
  benign, qw_neg  0.69 / 0.004 / 1.0 / 4.0 / 4.1                    2.0     2.2     4.0 / 5.2          5.3 / 5.9
  counts 1..400   1.0 / 0.5 / 1.7 / 48 / 42 (n = 400; sum_dt 47)    2.1     2.3     6.8 / 11 (n >= 7)  6.8 / 7.4 (n >= 7)
  dt (spread, 0)  2.2 / 0.05 / 0.94 / 1.6 / 3.4                     1.5     2.7     2.8 / 3.1          4.5 / 3.9
  high_dynamics   0.64 / 0.5 / 0.78 / 2.0 / 3.6                     1.0     2.0     3.9 / 5.5          4.5 / 4.6
  standstill      0.71 / 0 / 1.1 / 1.0 / 2.7                        0.2     0.2     0.8 / 2.9          1.7 / 2.4
  rot_near_pi     1.0 / 0.5 / 0.65 / 3.0 / 4.0                      1.5     1.7     2.7 / 7.1          3.1 / 3.3
  bias_far        1.0 / 0.5 / 0.65 / 2.7 / 3.6                      0.8     1.6     3.8 / 3.8          3.7 / 5.0
  noise           1.0 / 0.5 / 0.63 / 3.0 / 3.5                      1.6     2.1     6.3 / 7.9          3.9 / 4.5
  (n1: whitening 4.5e15 / 4.5e15, Gram 5.7e15 / 5.7e15 -- the singular covariance.)  The first-order rotation rows equal the oracle's bit for bit.

  projection family   residual (pair / per-residual form)   Jacobian (pair / per-residual)   Cauchy rows   weight
  draws               1.6 / 2.5                             6.6 / 7.0                        6.3           1.0
  tr x row            1.2 / 2.7                             4.7 / 5.5                        4.7           0
  invdep              1.8 / 2.1                             2.6 / 3.7                        3.0           0.85
  depj                1.3 / 1.1                             2.1 / 1.9                        2.1           0
  zero_baseline       2.5 / 1.7                             5.4 / 4.9                        5.1           0
  qw_neg              0.62 / 1.9                            1.4 / 4.6                        1.8           0.80
  rot179              3.9 / 1.3                             4.2 / 3.5                        3.1           0.60
  far_origin          0.0007 / 0.36                         0.008 / 0.43                     0.007         0.99
  ex (identity, default)  2.3 / 1.3                         2.8 / 3.2                        3.1           0.56
  cauchy (|r| 0, 1, 307)  2.3 / 2.3                         4.2 / 4.1                        4.3           0.71
  pose operations: Plus 1.1, prior delta 0.36 (all in units of eps scale; the bound is 64); round trip pose_dx(Plus(x0, d), x0) 1.8 (two chained
  operations, bound 192, derived where it is asserted).
"""
import ctypes as C

import numpy as np
import pytest

import factor_cases as fc
import factor_ref as fr

pytestmark = pytest.mark.gpu

SHORT, FACTOR, FLOOR = 64.0, 4.0, 16.0
IMU = sorted(fc.imu_cases())
PROJ = sorted(fc.proj_cases())
SENT = -7.25e77     # sentinel for buffers the routines write into


def _p(a):
    return a.ctypes.data


def _log(kind, name, **kw):
    print("MEASURED %s %s %s" % (kind, name, " ".join("%s=%.3g" % (k, v) for k, v in kw.items())))


# ------------------------------------------------------------------------------------------------ device runs, once per case
_pre_cache, _raw_cache = {}, {}


def dev_preint(P, name, mode, case=None):
    key = (name, mode)
    if key not in _pre_cache:
        c = case or fc.imu_cases()[name]
        cfg = P.default_config(**c["cfg_kw"])
        out, nb, buf = np.full(686, np.nan), C.c_int(-1), np.full((64, 7), np.nan)
        dt, acc, gyr = (np.ascontiguousarray(c[k], np.float64) for k in ("dt", "acc", "gyr"))
        rc = P.lib().vio_stage_preint(C.byref(cfg), mode, c["n"], _p(dt), _p(acc), _p(gyr), _p(c["acc0"]), _p(c["gyr0"]), _p(c["ba"]), _p(c["bg"]),
                                      _p(out), C.addressof(nb), _p(buf))
        assert rc == 0
        _pre_cache[key] = (out, nb.value, buf)
    return _pre_cache[key]


def dev_raw(P, name):
    """raw residual, raw Jacobian whole and by parts, on the device's own step-by-step pre-integration"""
    if name not in _raw_cache:
        c = fc.imu_cases()[name]
        cfg = P.default_config(**c["cfg_kw"])
        pre461 = np.ascontiguousarray(dev_preint(P, c.get("twin_of", name), 0)[0][:461])
        r, J, Jp = np.full(15, np.nan), np.full(450, np.nan), np.full(465, SENT)
        rc = P.lib().vio_stage_imu_raw(C.byref(cfg), _p(pre461), _p(c["ba"]), _p(c["bg"]), _p(c["pi"]), _p(c["sbi"]), _p(c["pj"]), _p(c["sbj"]), _p(r), _p(J),
                                       _p(Jp))
        assert rc == 0
        _raw_cache[name] = (pre461, r, J.reshape(15, 30), Jp.reshape(15, 31))
    return _raw_cache[name]


# ------------------------------------------------------------------------------------------------ pre-integration
@pytest.mark.parametrize("name", [n for n in IMU if "twin_of" not in fc.imu_cases()[n]])
def test_preintegration_both_routines_against_the_reference(P, orc, name):
    """preint_propagate step by step and preint_propagate_many (append off and on) return the same bits -- the claim of the latter's comment -- and
    agree with the reference per block; append files the first 64 samples and saturates n_buf."""
    c = fc.imu_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    ref = fc.imu_preint_ref(name)
    o0, nb0, buf0 = dev_preint(P, name, 0)
    o1, nb1, buf1 = dev_preint(P, name, 1)
    o2, nb2, buf2 = dev_preint(P, name, 2)
    assert np.isfinite(o0[:461]).all()
    assert o0.tobytes() == o1.tobytes() == o2.tobytes(), np.abs(o0 - o1).max()
    assert nb0 == 0 and nb1 == 0 and not buf0.any() and not buf1.any()
    k = min(c["n"], fc.SLOT_CAP)
    assert nb2 == k and not buf2[k:].any()
    assert np.array_equal(buf2[:k], np.c_[c["dt"], c["acc"], c["gyr"]][:k])
    orc_pre = fc.OraclePreint(orc, cfg, c)
    Ro, Rd = fc.preint_ratios(orc_pre.get(), ref), fc.preint_ratios(o0[:461], ref)
    orc_pre.close()
    _log("preint", name, **{k + s: float(np.max(R[k])) for k in ("dp", "dq", "dv", "sum_dt", "jac", "cov") for s, R in (("_dev", Rd), ("_orc", Ro))})
    for k in ("dp", "dq", "dv", "sum_dt", "jac", "cov"):
        assert np.all(Rd[k] <= FACTOR * Ro[k] + FLOOR), (k, Rd[k], Ro[k])
    assert abs(np.linalg.norm(o0[3:7]) - 1) <= 4 * fr.EPS     # normalised after every step
    if name == "dt_zero":   # a duplicated stamp changes neither the Jacobian nor the covariance (nor anything but the re-normalised delta_q)
        short = dev_preint(P, name + "/without_last", 0, fc.without_last(c))[0]
        assert fc.same_but_dq(o0[:461], short[:461])


# ------------------------------------------------------------------------------------------------ what be_ingest adds: the ring and the world state
# Ps / Rs / Vs after the n samples against factor_ref.process_imu, in units of eps x the largest term that entered the quantity.  The oracle's
# processIMU is a member of its estimator and cannot be driven on a state of the test's choosing, so the bars are ten times what was measured
# on an MI355X, rounded up to one digit (the rule of test_gpu_backend_edges.BARS); a measured 0 stands for itself.
WORLD_BARS = {          # n: (P, R, V)
    1:  (0, 6, 0),      # measured P 0     R 0.591 V 0
    2:  (7, 6, 0),      # measured P 0.635 R 0.589 V 0
    7:  (20, 20, 7),    # measured P 1.27  R 1.18  V 0.674
    8:  (20, 20, 10),   # measured P 1.27  R 1.18  V 0.972
    9:  (20, 20, 20),   # measured P 1.9   R 1.76  V 1.25
    16: (30, 20, 20),   # measured P 2.54  R 1.76  V 1.2
    17: (20, 20, 20),   # measured P 1.9   R 1.76  V 1.16
    63: (50, 30, 20),   # measured P 4.44  R 2.92  V 1.87
    64: (60, 30, 30),   # measured P 5.08  R 2.92  V 2.23
    65: (40, 50, 30),   # measured P 3.81  R 4.09  V 2.2
}


def dev_ring(P, n):
    c = fc.ring_case(n)
    cfg = P.default_config(**c["cfg_kw"])
    out, nb, buf = np.full(686, np.nan), C.c_int(-1), np.full((64, 7), np.nan)
    world = np.r_[c["acc0"], c["gyr0"], c["Ps"], c["Vs"], c["Rs"].ravel(), c["ba"], c["bg"], c["g"], np.nan]
    rc = P.lib().vio_stage_preint_ring(C.byref(cfg), n, c["head"], fc.RING_CAP, _p(c["ring_t"]), _p(c["ring_acc"]), _p(c["ring_gyr"]), c["prev"], c["cur"],
                                       _p(world), _p(c["acc0"]), _p(c["gyr0"]), _p(c["ba"]), _p(c["bg"]), _p(out), C.addressof(nb), _p(buf))
    assert rc == 0
    return out, nb.value, buf, world


@pytest.mark.parametrize("n", fc.RING_COUNTS)
def test_ingest_propagation_on_a_ring_with_the_world_state(P, n):
    """be_ingest's use of preint_propagate_many -- the interval of a wrapping ring as the sample source, dt formed on the device, the world-state
    step of processIMU as the side job -- returns the bits of the merge's use (mode 2) fed numpy's dt, files the same buffer, raises overflow
    bit 2 exactly when more than 64 samples were filed, and moves Ps / Rs / Vs as estimator.cpp:142-152 does."""
    c = fc.ring_case(n)
    ts = np.sort(c["ring_t"][np.isfinite(c["ring_t"])])
    assert c["head"] + n > fc.RING_CAP and len(ts) == n and c["prev"] < ts[0] and (n < 2 or ts[-2] < c["cur"] < ts[-1])
    out, nb, buf, world = dev_ring(P, n)
    o2, nb2, buf2 = dev_preint(P, c["name"], 2, c)
    assert np.isfinite(out).all() and out.tobytes() == o2.tobytes(), np.abs(out - o2).max()
    assert nb == nb2 == min(n, fc.SLOT_CAP) and buf.tobytes() == buf2.tobytes()
    assert np.array_equal(buf[:nb], np.c_[c["dt"], c["acc"], c["gyr"]][:nb]) and not buf[nb:].any()
    assert world[30] == (2.0 if n > fc.SLOT_CAP else 0.0)
    assert np.array_equal(world[0:3], c["acc"][n - 1]) and np.array_equal(world[3:6], c["gyr"][n - 1])
    assert np.array_equal(world[21:30], np.r_[c["ba"], c["bg"], c["g"]])
    ref = fr.process_imu(c["dt"], c["acc"], c["gyr"], c["acc0"], c["gyr0"], c["Ps"], c["Rs"], c["Vs"], c["ba"], c["bg"], c["g"])
    e = (np.abs(world[6:9] - ref["P"]).max() / (fr.EPS * ref["scale_p"]), np.abs(world[12:21].reshape(3, 3) - ref["R"]).max() / (fr.EPS * ref["scale_r"]),
         np.abs(world[9:12] - ref["V"]).max() / (fr.EPS * ref["scale_v"]))
    _log("world", c["name"], P=e[0], R=e[1], V=e[2])
    bP, bR, bV = WORLD_BARS[n]
    assert e[0] <= bP and e[1] <= bR and e[2] <= bV, (e, WORLD_BARS[n])


# ------------------------------------------------------------------------------------------------ raw residual and Jacobian
@pytest.mark.parametrize("name", IMU)
def test_raw_imu_residual_and_jacobian(P, orc, name):
    """imu_raw_residual, imu_raw_jacobian and the four imu_raw_jacobian_part calls, entry by entry, on the device's own pre-integration taken as
    float64 input.  The exact blocks and (where Bg_i = bg) the rotation rows against the derivative; the first-order rotation rows elsewhere
    against upstream's formula in extended precision and against the oracle's raw rows on the same pre-integration."""
    c = fc.imu_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    pre461, r, J, Jp = dev_raw(P, name)
    pre = fr.pre_from_461(pre461, c["ba"], c["bg"])
    a = (pre, cfg.g_norm, c["pi"], c["sbi"], c["pj"], c["sbj"])
    rr, rs = fr.imu_residual(*a)
    Jf, Js = fr.imu_jacobian_formula(*a)
    Jd = fr.imu_jacobian_derivative(*a)
    o = fc.OraclePreint(orc, cfg, c, push=False)
    o.set_state(pre461)
    ro, Jo = o.raw()
    o.close()
    deriv = ~fr.IMU_ZERO & (~fr.IMU_ROT_ROWS | c["dbg0"])
    first = ~fr.IMU_ZERO & ~deriv
    e_r = fr.ratio(r, rr, rs).max()
    assert np.array_equal(Jp[:, 30], np.full(15, SENT))
    worst = {}
    for tag, Jx in (("whole", J), ("parts", Jp[:, :30])):
        assert not Jx[fr.IMU_ZERO].any()
        worst[tag + "_deriv"] = fr.ratio(Jx, Jd, Js, fr.DIFF_SLACK)[deriv].max()
        worst[tag + "_formula"] = fr.ratio(Jx, Jf, Js).max()
        worst[tag + "_oracle_rot"] = fr.ratio(Jx, Jo, Js)[first].max() if first.any() else 0.0
    _log("imu_raw", name, residual=e_r, **worst)
    assert e_r <= SHORT
    assert max(worst.values()) <= SHORT, worst
    if name == "standstill":
        assert np.abs(r).max() <= SHORT * fr.EPS * rs.max()


# ------------------------------------------------------------------------------------------------ whitening and the Gram matrix
@pytest.mark.parametrize("name", IMU)
def test_whitening_and_gram_matrix(P, orc, name):
    """M = chol(cov)^-1 of preint_store against the device's own covariance (M cov M^T = I in mpmath), and the 31 x 31 Gram matrix of
    imu_block_mfma against [J r]^T cov^-1 [J r] formed in mpmath from the device's raw J, r and covariance: the whitening and matrix-core step
    alone.  Yardstick: the oracle's LLT(cov^-1) route on the same covariance and the same raw J, r."""
    c = fc.imu_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    base = c.get("twin_of", name)
    pre461, r, J, _ = dev_raw(P, name)
    M = dev_preint(P, base, 0)[0][461:].reshape(15, 15)
    cov = pre461[236:].reshape(15, 15)
    assert np.isfinite(M).all() and not np.triu(M, 1).any()
    o = fc.OraclePreint(orc, cfg, c, push=False)
    o.set_state(pre461)
    o_sqrt = o.sqrt_info()
    wh_o = fr.whiten_identity_error(o_sqrt, cov) / fr.EPS
    ro, Jo = o.raw()
    rw, Jw = o.whitened()
    o.close()
    A = np.hstack([Jw, rw[:, None]])
    g_o = fc.gram_scaled_error(A.T @ A, fr.gram_ref(Jo, ro, cov))
    wh_d = fr.whiten_identity_error(M, cov) / fr.EPS
    G = np.full((31, 31), np.nan)
    dt, acc, gyr = (np.ascontiguousarray(c[k], np.float64) for k in ("dt", "acc", "gyr"))
    rc = P.lib().vio_stage_imu_block(C.byref(cfg), c["n"], _p(dt), _p(acc), _p(gyr), _p(c["acc0"]), _p(c["gyr0"]), _p(c["ba"]), _p(c["bg"]), _p(c["pi"]),
                                     _p(c["sbi"]), _p(c["pj"]), _p(c["sbj"]), _p(G))
    assert rc == 0 and np.isfinite(G).all()
    assert np.array_equal(G, G.T)
    g_d = fc.gram_scaled_error(G, fr.gram_ref(J, r, cov))
    _log("whiten", name, identity_dev=wh_d, identity_orc=wh_o, gram_dev=g_d, gram_orc=g_o)
    assert wh_d <= FACTOR * wh_o + FLOOR
    assert g_d <= FACTOR * g_o + FLOOR
    if name == "n1":
        # the singular one-step covariance has no usable Cholesky factor: both sides say so by an all-zero whitening matrix (include/vio_abi.h,
        # vio_stage_preint), and the factor then contributes exactly nothing to the normal equations
        assert not o_sqrt.any() and not M.any() and not G.any()
    else:
        assert M.diagonal().min() > 0 and o_sqrt.any()


# ------------------------------------------------------------------------------------------------ projection
def _dev_proj(P, fn, cfg, c, use_td):
    r, J = np.full(2, np.nan), np.full(46, np.nan)
    assert fn(C.byref(cfg), _p(c["pi"]), _p(c["pj"]), _p(c["ex"]), c["inv_dep"], c["td"], _p(c["oi"]), _p(c["oj"]), use_td, _p(r), _p(J)) == 0
    return r, fc.j20_of_46(J)


def _dev_pair(P, cfg, c, use_td, cauchy, rs, ext, nJ=48):
    r, w, J = np.full(2, np.nan), np.full(1, SENT), np.full(nJ, SENT)
    rc = P.lib().vio_stage_projection_pair(C.byref(cfg), _p(c["pi"]), _p(c["pj"]), _p(c["ex"]), c["inv_dep"], c["td"], _p(c["oi"]), _p(c["oj"]), use_td,
                                           cauchy, rs, ext, _p(r), _p(w), _p(J), nJ)
    assert rc == 0
    return r, w[0], J


@pytest.mark.parametrize("use_td", [0, 1])
@pytest.mark.parametrize("name", PROJ)
def test_projection_both_forms_weight_and_compact_rows(P, name, use_td):
    """eval_projection and eval_projection_pair: residual and all 20 columns against the reference; the Cauchy-weighted rows are s times the unweighted
    reference rows with s = 1 / sqrt(1 + |r|^2) from mpmath; the compact rows and the rows without the extrinsic block are the full rows' columns,
    bit for bit, with every element they do not own left as it was."""
    c = fc.proj_cases()[name]
    cfg = P.default_config(**c["cfg_kw"])
    K = fr.proj_consts(cfg)
    a = (c["pi"], c["pj"], c["ex"], c["inv_dep"], c["td"], c["oi"], c["oj"], use_td)
    rr, rs_ = fr.proj_residual(K, *a)
    Jd = fr.proj_jacobian_derivative(K, *a)
    _, Js = fr.proj_jacobian_formula(K, *a)
    worst = {}
    for tag, fn in (("pair", P.lib().vio_stage_projection), ("residual", P.lib().vio_stage_projection_residual)):
        r, J = _dev_proj(P, fn, cfg, c, use_td)
        worst[tag + "_r"] = fr.ratio(r, rr, rs_).max()
        worst[tag + "_J"] = fr.ratio(J, Jd, Js, fr.DIFF_SLACK).max()
        if not use_td:
            assert not J[:, 18].any()
    full = {}
    for cauchy in (0, 1):
        r, w, J = _dev_pair(P, cfg, c, use_td, cauchy, 20, 1)
        assert np.array_equal(J[40:], np.full(8, SENT))
        J = J[:40].reshape(2, 20)
        full[cauchy] = J
        if not use_td:
            assert not J[:, 18].any()
        if cauchy:
            s = fr.cauchy_weight(r)
            worst["weight"] = abs(w - s) / (fr.EPS * s)
            worst["cauchy_J"] = fr.ratio(J, s * Jd, s * Js, fr.DIFF_SLACK).max()
        else:
            assert w == SENT
            worst["stage_r"] = fr.ratio(r, rr, rs_).max()
            worst["stage_J"] = fr.ratio(J, Jd, Js, fr.DIFF_SLACK).max()
        # compact rows: [pose_i pose_j inv_depth -]; slot 13 of either row and everything past the rows untouched
        r14, w14, J14 = _dev_pair(P, cfg, c, use_td, cauchy, 14, 0)
        assert np.array_equal(r14, r) and w14 == w
        rows = J14[:28].reshape(2, 14)
        assert np.array_equal(rows[:, :12], J[:, :12]) and np.array_equal(rows[:, 12], J[:, 19])
        assert np.array_equal(rows[:, 13], [SENT, SENT]) and np.array_equal(J14[28:], np.full(20, SENT))
        # full-width rows of a solve with constant extrinsic and td: columns 0 .. 11 and the inverse depth at 12, the rest untouched
        r20, w20, J20 = _dev_pair(P, cfg, c, use_td, cauchy, 20, 0)
        rows = J20[:40].reshape(2, 20)
        assert np.array_equal(r20, r) and w20 == w
        assert np.array_equal(rows[:, :12], J[:, :12]) and np.array_equal(rows[:, 12], J[:, 19])
        assert np.array_equal(rows[:, 13:], np.full((2, 7), SENT)) and np.array_equal(J20[40:], np.full(8, SENT))
    _log("projection", "%s/td%d" % (name, use_td), r_norm=float(np.linalg.norm(rr)), **worst)
    assert max(worst.values()) <= SHORT, worst


def test_projection_pair_stage_rejects_layouts_the_routine_does_not_have(P):
    c = fc.proj_cases()["draw0"]
    cfg = P.default_config()
    r, w, J = np.zeros(2), np.zeros(1), np.full(48, SENT)
    for rs, ext, nJ in ((14, 1, 48), (16, 0, 48), (20, 1, 39), (14, 0, 27)):
        assert P.lib().vio_stage_projection_pair(C.byref(cfg), _p(c["pi"]), _p(c["pj"]), _p(c["ex"]), c["inv_dep"], c["td"], _p(c["oi"]), _p(c["oj"]), 0, 0,
                                                 rs, ext, _p(r), _p(w), _p(J), nJ) != 0
    assert np.array_equal(J, np.full(48, SENT))


# ------------------------------------------------------------------------------------------------ pose operations
def _pose_ops(P, x, d, x0):
    x, d, x0 = (np.ascontiguousarray(v, np.float64) for v in (x, d, x0))
    plus, dx = np.full((len(x), 7), np.nan), np.full((len(x), 6), np.nan)
    assert P.lib().vio_stage_pose_ops(len(x), _p(x), _p(d), _p(x0), _p(plus), _p(dx)) == 0
    return plus, dx


def test_pose_plus_and_prior_delta(P):
    names, x, d = fc.plus_cases()
    plus, _ = _pose_ops(P, x, d, x)
    worst = {}
    for i, n in enumerate(names):
        v, s = fr.pose_plus(x[i], d[i])
        worst["plus_" + n] = fr.ratio(plus[i], v, s).max()
        assert abs(np.linalg.norm(plus[i][3:]) - 1) <= 4 * fr.EPS
    names, x, x0, flip = fc.delta_cases()
    _, dx = _pose_ops(P, x, np.zeros((len(x), 6)), x0)
    for i, n in enumerate(names):
        v, s, w = fr.pose_delta(x[i], x0[i])      # v carries the sign rule applied to the exact w
        worst["delta_" + n] = fr.ratio(dx[i], v, s).max()
    _log("pose", "ops", **worst)
    assert max(worst.values()) <= SHORT, worst
    i = names.index
    # the flip happens exactly where the rule says: not at w = 0, at the first negative w
    assert np.array_equal(dx[i("w_exactly_0")][3:], [2, 0, 0]) and dx[i("w_slightly_neg")][3] < -1.9 and dx[i("w_slightly_pos")][3] > 1.9
    assert np.abs(dx[i("near")][3:] - dx[i("near_negated")][3:]).max() <= SHORT * fr.EPS     # q and -q are the same rotation: the same delta
    assert not dx[i("x_eq_x0")][:3].any() and np.abs(dx[i("x_eq_x0")][3:]).max() <= SHORT * fr.EPS
    # round trip: rotation part of pose_dx(Plus(x0, d), x0) = d / sqrt(1 + |d|^2 / 4).  Two operations: Plus errs by <= 64 eps on a unit
    # quaternion, the delta map 2 vec(q0^-1 q) doubles that and adds its own 64 eps: 192 eps on a scale of max(1, |result|)
    D = fc.ROUND_TRIP_D
    x0 = np.tile(fc.plus_cases()[1][0], (len(D), 1))
    plus, _ = _pose_ops(P, x0, D, x0)
    _, dx = _pose_ops(P, plus, np.zeros_like(D), x0)
    rt = []
    for k in range(len(D)):
        want = D[k][3:] / np.sqrt(1 + D[k][3:] @ D[k][3:] / 4)
        rt.append(np.abs(dx[k][3:] - want).max() / (fr.EPS * max(1.0, np.abs(want).max())))
        assert np.abs(dx[k][:3] - D[k][:3]).max() <= 4 * fr.EPS * max(1.0, np.abs(x0[k][:3] + D[k][:3]).max())
    _log("pose", "round_trip", worst=max(rt))
    assert max(rt) <= 192, rt
