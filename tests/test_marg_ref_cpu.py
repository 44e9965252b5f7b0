"""tests/marg_ref.py against itself, without a GPU: the two routes to A_mm^+ agree, the float64 numpy evaluation of the literal algorithm
(numpy.linalg.eigh) stays inside every bound on every input tests/test_gpu_marg_literal.py uses, the certificate's inputs leave no case between
"must certify" and "must refuse", and the window_size = 20 stream of the pipeline tests reaches the marginalisation it is there for.

The routes.  `block_inverse` run on mpmath numbers agrees with the eigsy route to 1e-25 relative; run in np.longdouble (64-bit mantissa, the
arithmetic the references beyond m = 32 use) it agrees to C m 2^-63 cond(A_mm), the most that format can give.

Worst error / bound of float64 numpy per family (the bound is wrong if one exceeds 1; test_zz_report_worst_ratios prints them):
    part 0  A_mm^+   well 0.056  asym 0.069  null 0.032  graded 0.0004   drop1 / drop3 / dropall 0.013 / 0.009 / 0.029   strict 0.0007  strict_general 0.016
            A_r      well 0.030  asym 0.045  null 0.028  graded < 1e-4   drops 0.005 / 0.001 / 0.016                      strict < 1e-4  strict_general 0.005
            b_r      well 0.020  asym 0.018  null 0.012  graded < 1e-4   drops 0.002 / 0.001 / 0.004                      strict < 1e-4  strict_general 0.002
            the prior that follows (all kept): prior_H 0.105, prior_r 0.024, prior_c0 0.014, J^T J / J^T rf / |rf|^2 0.106 / 0.035 / 0.061
    part 1  prior_H  kept 0.083  null 0.037  gauge 0.125  neg 0.125      prior_r <= 0.046                                 prior_c0 <= 0.052
            J^T J / J^T rf / |rf|^2 against the returned H / r / c0: 0.384 / 0.390 / 0.346 (at n = 1: one rounding against gamma_1), <= 0.05 from n = 22 on
    part 2  bound against its long-double value: 0.012 of C (F0 + md) eps
"""
import numpy as np
import pytest

import backend_cases as BC
import linalg_ref as R
import marg_ref as M

_worst = {}


def _note(fam, ratios):
    for k, v in ratios.items():
        if k != "rows":
            _worst[(fam, k)] = max(_worst.get((fam, k), 0.0), float(v))


# ------------------------------------------------------------------------------------------------------------- the two routes to A_mm^+
@pytest.mark.parametrize("md,F0", [(6, 0), (15, 0), (15, 1), (15, 2), (15, 16), (15, 17)])
def test_eigsy_route_and_block_elimination_agree(md, F0):
    import mpmath
    for kind in [k for k in M.part0_kinds(md, F0) if k in ("well", "asym", "graded", "drop1", "dropall", "drop3")]:
        s = M.part0_case(kind, md, F0, M.P0_N)
        ref = M.ref_part0(s, "mp")
        Pm, B, d = s.parts()[:3]
        keep = np.concatenate([np.ones(md, bool), d > M.CUT])
        assert ref.n_dropped == int((~keep).sum()), kind
        with mpmath.workdps(R.DPS):
            Xe = M.block_inverse(M.to_mp(Pm), M.to_mp(B[keep[md:]]), M.to_mp(d[keep[md:]]))
            Xmp = ref.X_mp[np.ix_(keep, keep)]
            scale = max(abs(x) for x in Xmp.reshape(-1))
            err = max(abs(a - b) for a, b in zip(Xe.reshape(-1), Xmp.reshape(-1))) / scale
            off = max([abs(x) for x in ref.X_mp[~keep].reshape(-1)], default=0)
        assert err <= 1e-25 and off <= 1e-25 * scale, (kind, md, F0, float(err), float(off))
        Xl, keep_l = M.pinv_ld(s)
        assert np.array_equal(keep_l, keep)
        dl = float(np.abs(Xl - ref.X).max()) / float(np.abs(ref.X).max())
        cond = ref.normA / ref.lam_kept_min
        assert dl <= M.C * s.m * 2.0 ** -63 * cond, (kind, md, F0, dl, cond)


# ------------------------------------------------------------------------------------------------------------- float64 numpy inside the bounds
def _check0(kind, md, F0, n):
    s = M.part0_case(kind, md, F0, n)
    ref = M.part0_ref(kind, md, F0, n)
    X, Ar, br = M.np_part0(s)
    ratios = M.check_part0(ref, X, Ar, br)
    _note("p0 " + kind, ratios)
    assert all(v <= 1.0 for v in ratios.values()), (kind, md, F0, n, ratios)
    if kind == "well":
        assert ref.normA / ref.lam_kept_min <= 1e3
    if kind.startswith("strict"):
        assert X[ref.i_lo, ref.i_lo] == 0.0 and not np.any(X[ref.i_lo]) and X[ref.i_hi, ref.i_hi] > 0.0
    return s, ref, (X, Ar, br)


@pytest.mark.parametrize("md,F0,n,mxl", M.part0_sizes() + [(15, 480, 76, 0)])
def test_numpy_part0_stays_inside_every_bound(md, F0, n, mxl):
    for kind in M.part0_kinds(md, F0):
        s, ref, (X, Ar, br) = _check0(kind, md, F0, n)
        # the prior that follows: on these inputs A_r is positive definite far above the cut (ref1_all_kept asserts it), so every direction is kept
        out = M.check_part1(M.ref1_all_kept(Ar, br), *M.np_part1(Ar, br))
        _note("p0 prior", out)
        assert out.pop("rows") == n and all(v <= 1.0 for v in out.values()), (kind, md, F0, out)


def test_dropping_every_landmark_leaves_the_pose_block_of_the_landmark_free_system():
    a, b = M.part0_ref("dropall", 15, 17, M.P0_N), M.part0_ref("well", 15, 0, M.P0_N)
    assert np.array_equal(M.part0_case("dropall", 15, 17, M.P0_N).A, M.part0_case("well", 15, 0, M.P0_N).A)
    assert float(np.abs(a.X[:15, :15] - b.X).max()) <= 1e-30 and not np.any(a.X[15:]) and not np.any(a.X[:, 15:])


@pytest.mark.parametrize("n", M.part1_sizes())
def test_numpy_part1_stays_inside_every_bound(n):
    for kind in M.PART1_KINDS:
        A, b, ref = M.part1_case(kind, n)
        out = M.check_part1(ref, *M.np_part1(A, b))
        _note("p1 " + kind, out)
        assert out.pop("rows") == ref.n_kept, (kind, n)
        assert all(v <= 1.0 for v in out.values()), (kind, n, out)
        lam = M.spectrum(kind, n) if kind != "null" else None
        if lam is not None:
            assert ref.n_kept == int((lam > M.CUT).sum())
            if np.any(lam <= M.CUT):
                assert lam[lam > M.CUT].min() >= 1e-6 and lam[lam <= M.CUT].max() <= 1e-10


@pytest.mark.parametrize("n", [2, 22, 32])
def test_construction_and_mpmath_references_of_the_second_half_agree(n):
    """where both apply they differ by the rounding of A_r to float64 (e_ref), which the construction route carries in its bounds"""
    for kind in M.PART1_KINDS:
        A, b, rc = M.reduced(kind, n)
        rm = M.ref1_mp(A, b)
        assert rm.n_kept == rc.n_kept
        e = rc.E - rm.E if kind != "null" else M.EPS * rc.normA
        k = rc.H_bound / rc.E
        assert M.norm2((rm.H - rc.H).astype(np.float64)) <= 2 * e * k, (kind, n)
        assert float(np.linalg.norm((rm.Pb - rc.Pb).astype(np.float64))) <= 2 * e * rc.r_bound / rc.E + 1e-300, (kind, n)
        assert abs(float(rm.c0 - rc.c0)) <= 2 * e * rc.c0_bound / rc.E, (kind, n)


def test_strictness_inputs_sit_on_the_cut():
    assert M.CUT == 1e-8 and not (M.CUT > 1e-8) and M.TWO_M26 > 1e-8 and M.TWO_M26 == 2.0 ** -26
    A, b = M.strict_diagonal(22)
    J, rf, H, r, c0 = M.np_part1(A, b)
    assert not np.any(J[0]) and rf[0] == 0.0 and J[1, 1] == 2.0 ** -13 and rf[1] == 2.0 * 2.0 ** 13
    s = M.part0_case("strict", 15, 17, M.P0_N)
    Amm = s.Amm()
    assert np.array_equal(Amm, np.diag(np.diag(Amm))) and s.d[-2] == 1e-8 and s.d[-1] == 2.0 ** -26


# ------------------------------------------------------------------------------------------------------------- the certificate
@pytest.mark.parametrize("md,F0", M.CERT_SIZES)
def test_certificate_inputs_leave_nothing_between_certify_and_refuse(md, F0):
    seen = set()
    for lam in M.CERT_SWEEP:
        c = M.cert_case(md, F0, lam)
        # the sweep value (set through a float64 eigvalsh, m eps |A_mm| ~ 1e-13 absolute), confirmed by mpmath / long double
        assert abs(c.lam_min - lam) <= 1e-3 * lam, (lam, c.lam_min)
        # the bound is one: 1 / |A^-1|_F <= lambda_min, up to the long-double inversion behind Pinv (C m 2^-63 cond <= 1e-6 at cond 1e10)
        assert c.inv_bound <= c.lam_min * (1 + 1e-6)
        assert c.inv_bound >= 2e-7 or c.inv_bound <= 0.5e-7, (md, F0, lam, c.inv_bound)
        ok, bound = M.np_cert(c.Pinv, c.Cl, c.dinv)
        assert ok == (c.inv_bound >= 2e-7)
        assert not ok or c.lam_min > 1e-7
        rel = abs(bound - float(c.bound)) / float(c.bound) / (M.C * (F0 + md) * M.EPS)
        _note("p2", {"bound": rel})
        assert rel <= 1.0
        seen.add(ok)
    assert seen == {True, False}


def test_certificate_refusals_in_numpy():
    c = M.cert_case(15, 17, 1e-3)
    assert M.np_cert(c.Pinv, c.Cl, c.dinv)[0]
    assert not M.np_cert(c.Pinv, c.Cl, c.dinv, pinv_direct=0)[0]
    for v in (0.0, -1.0):
        dinv = c.dinv.copy()
        dinv[5] = v
        assert not M.np_cert(c.Pinv, c.Cl, dinv)[0]
    Pn = c.Pinv.copy()
    Pn[3, 4] = np.nan
    assert not M.np_cert(Pn, c.Cl, c.dinv)[0]
    assert M.np_cert(c.Pinv, np.full_like(c.Cl, np.nan), np.full_like(c.dinv, np.nan), second_new=True)[0]


# ------------------------------------------------------------------------------------------------------------- the 20-frame window
def test_w20_stream_initialises_and_marginalises_the_oldest_frame(P, orc):
    st = BC.w20_moving(P)
    recs = BC.run_oracle(st)
    W = st.cfg.window_size
    assert W == 20 and 6 * W + 16 == 136 and len(recs) == W + 14
    assert [int(r["status"]["solver_flag"]) for r in recs] == [0] * W + [1] * 14
    assert all(r["rc"] == 1 and int(r["status"]["reboot_count"]) == 0 for r in recs)
    old = [k for k in range(W + 1, len(recs)) if int(recs[k]["status"]["marginalization_flag"]) == 0 and int(recs[k]["status"]["has_prior"]) == 1]
    assert len(old) >= 5, old
    assert all(BC.anchored(recs[k - 1]) >= 40 for k in old)


def test_zz_report_worst_ratios():
    """(prints what the module docstring records; run with -s)"""
    for k in sorted(_worst):
        print("%-22s %-6s %.4f" % (k[0], k[1], _worst[k]))
