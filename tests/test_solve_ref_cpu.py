"""tests/solve_ref.py against itself, without a GPU: every case of tests/test_gpu_solve_stage.py reaches the edge it is named for (on the reference
alone), the reference's own caps hold, float64 numpy of the same definition lies inside every derived bound, and the long-double and mpmath routes
agree.

Worst error / bound of float64 numpy (residuals summed in a shuffled order, numpy.linalg.solve) over all cases (test_zz_report_worst_ratios prints
them): H 0.011, g 4.6e-4, Hpl 7.3e-4, Hll 1.6e-4, gl 7.9e-4, cost 0.0015, Gauss-Newton residual 1.4e-4, forward error 6.5e-6.
The measurement behind the bars of the dogleg quantities (solve_ref docstring, (c)): float64 numpy with the factors moved by their factor-level bound
differs from the reference by 1e-11 .. 5.7e-2 of the largest step entry, median 5e-7 (the float64 difference itself, no derived bound mixed in)."""
import numpy as np
import pytest

import marg_default_ref as D
import solve_ref as R

L = np.longdouble
NAMES = sorted(R.CASES)
_worst = {}
_steps = {}


def _cfg(P, name):
    return P.canonical_config(**R.cfg_kwargs(name))


def _at_x0(P, name):
    cfg = _cfg(P, name)
    pb = R.get_problem(name, cfg)
    X, feat = pb.x0()
    lin, st = R.lin_at(name, cfg, X, feat)
    return cfg, pb, X, feat, lin, st


def test_case_list_covers_the_sizes_and_kinds(P):
    assert {R.CASES[n][0]["W"] for n in NAMES} == {4, 10, 11, 20}
    pbs = {n: R.get_problem(n, _cfg(P, n)) for n in NAMES}
    assert {pbs["Fa%d_W4" % f].Fa for f in (0, 1, 3, 4, 5, 16, 17)} == {0, 1, 3, 4, 5, 16, 17}
    assert all(pbs["Fa%d_W4" % f].F == 19 for f in (0, 1, 3, 4, 5, 16, 17))            # all landmarks constant against F > 0 included
    for n in (251, 252, 253, 255, 256, 257, 511, 512, 513):
        assert pbs["nres%d_W4" % n].nres == n
    assert 252 == R.PS_FUSE_CAP - 4                                                     # a chunk boundary of the fused kernel at W = 4
    assert max(pbs["pair64_W10"].pair_counts.values()) == 64 and max(pbs["pair65_W10"].pair_counts.values()) == 65
    W1 = 11
    assert len(pbs["pair64_W10"].pair_counts) < W1 * 10 // 2                            # frame pairs without a residual
    pb = pbs["two_frames_W10"]
    assert sum(1 for s in pb.plist if pb.st["lm_nobs"][s] == 2) >= 2
    assert pbs["big_W20"].F <= 24 and pbs["big_W11"].W == 11
    assert pbs["no_prior_W4"].st["prior"] is None and not pbs["absent_W10"].st["prior"]["present"].all()
    assert pbs["ex_td_fast_W4"].ex_active and pbs["ex_td_fast_W4"].td_active and pbs["ex_td_fast_W4"].vext
    assert not pbs["ex_td_slow_W4"].ex_active and not pbs["ex_td_slow_W4"].td_active
    assert 0.1 < np.linalg.norm(pbs["ex_td_slow_W4"].st["Vs"][0]) < 0.2 < np.linalg.norm(pbs["ex_td_fast_W4"].st["Vs"][0])
    assert not pbs["no_imu_W4"].use_imu and len(pbs["no_imu_W4"].act) == 6 * 4
    assert pbs["bounded_W4"].constrained and len(pbs["bounded_W4"].bounded) == 2
    assert pbs["noshuffle_W4"].plist == sorted(pbs["noshuffle_W4"].plist) and pbs["base_W10"].plist != sorted(pbs["base_W10"].plist)
    assert all(pbs[n].st["ring_base"] != 0 for n in NAMES if n != "noshuffle_W4")


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge_and_float64_stays_inside(P, name):
    cfg, pb, X, feat, lin, st = _at_x0(P, name)
    kw = R.CASES[name][0]
    assert lin.terms * R.EPS < 1e-11
    if kw.get("long_dt"):
        assert lin.sum_dt[0] > 10.0 and max(lin.sum_dt[1:]) < 1.0
    elif pb.use_imu:
        assert max(lin.sum_dt) < 1.0
    if kw.get("outlier"):
        assert min(lin.weights) < 0.05
    if kw.get("flat"):
        assert float(st.Dg[st.na:].min()) == 1e-3 and float(D._f64(lin.Hll).min()) < 1e-20      # the clamp at 1e-6 is active
    # ---- float64 numpy of the same definition, unperturbed factors, inside the derived bounds
    e = R.np_step(pb, X, feat, R.RADIUS0, 7, perturb=False)
    ix = np.ix_(pb.act, pb.act)
    q = dict(H=R.ratio(e["lin"].H[ix], lin.H[ix], lin.EH[ix]), g=R.ratio(e["lin"].g[pb.act], lin.g[pb.act], lin.Eg[pb.act]),
             cost=R.ratio(e["lin"].cost, lin.cost, lin.cost_bound))
    if pb.Fa:
        q.update(Hpl=R.ratio(e["lin"].Hpl, lin.Hpl, lin.EHpl), Hll=R.ratio(e["lin"].Hll, lin.Hll, lin.EHll), gl=R.ratio(e["lin"].gl, lin.gl, lin.Egl))
    y = e["y_gn"]
    q["gn_residual"] = float(np.max(np.abs(D._f64(st.M @ y.astype(L) - st.gs)) / st.res_bound_of(np.abs(y))))
    assert st.fwd_bounded == (name not in R.FWD_UNBOUNDED), (name, st.rho_fwd)
    if st.fwd_bounded:
        q["gn_forward"] = R.ratio(y, st.y, st.y_bound)
    for k, v in q.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    assert max(q.values()) <= 1.0, (name, q)
    # ---- the three branches and the step control
    rr, r1, r2 = R.radii(st)
    assert (rr["interp"] is None) == (name in R.NO_INTERP), (name, r1, r2)
    f0 = lin.cost
    seen = {}
    for branch, radius in rr.items():
        if radius is None:
            continue
        bar, d = R.bars(pb, X, feat, st, radius)
        assert d["branch"] == branch
        if branch != "gn":
            assert radius <= 0.5 * r1 and (radius >= 2 * r2 if branch == "interp" else radius <= 0.5 * r2)
        assert float(d["model_change"]) > 0
        zmax = float(np.max(np.abs(d["z"])))
        _steps.setdefault("step_bar_rel", []).append(bar["z_measured"] / zmax)
        Xc, cf, _, delta, dl = R.candidate(pb, X, feat, st.s, d["y"])
        fc, efc = R.cost(pb, Xc, cf)
        ok, newr, rho = R.step_control(f0, fc, d["model_change"], radius, float(d["norm"]))
        seen[branch] = ok
        # a factor 2 from the thresholds 1e-3 and 0.25 of the step control; from 0.75 as far as a ratio can be that is 1 for a quadratic cost
        # (0.93 .. 1.07 on every case with a prior or an IMU): 0.1; every distance at least 100 times the error the bounds leave in the ratio
        for thr in (R.MIN_REL_DECREASE, 0.25):
            assert not (0.5 * thr <= rho <= 2 * thr), (name, branch, rho)
        assert abs(rho - 0.75) >= 0.1, (name, branch, rho)
        rho_err = (lin.cost_bound + efc) / float(d["model_change"]) + abs(rho) * bar["model_change"] / float(d["model_change"])
        assert rho_err <= 1e-2 * min(abs(rho - t) for t in (R.MIN_REL_DECREASE, 0.25, 0.75)), (name, branch, rho, rho_err)
        assert abs(float(f0 - fc)) > 2e-6 * float(f0)
        xn = np.sqrt(sum(float(np.sum(X[k][:pb.W1] ** 2)) for k in ("pose", "sb")))
        assert float(np.linalg.norm(np.r_[delta, dl])) > 2e-8 * (xn + 1e-8)
        assert efc < 1e-3 * abs(float(f0 - fc)) or not ok
    if R.CASES[name][2].get("reject"):
        assert seen["gn"] is False, "the scanned perturbation must give a rejected full step"


def test_constrained_case_makes_the_line_search_backtrack(P):
    """bounded_reject_W4: the full step, projected onto the box, misses the Armijo condition by the definition, so the accepted a is below 1
    (bounded_W4's full step leaves the box and is cut back onto it, but satisfies the condition there: a = 1)"""
    cfg, pb, X, feat, lin, st = _at_x0(P, "bounded_reject_W4")
    assert pb.constrained
    d = R.dogleg(st, R.RADIUS0)
    Xc, cf, _, delta, dl = R.candidate(pb, X, feat, st.s, d["y"])
    fc, efc = R.cost(pb, Xc, cf)
    gd = float(D._f64(lin.g[pb.act]) @ delta[pb.act] + D._f64(lin.gl) @ dl)
    print("bounded_reject_W4 full step: f0 %.6g f %.6g g.d %.6g box %s" % (float(lin.cost), float(fc), gd, [float(feat[pb.var[a]] + dl[a] - pb.ub) for a in pb.bounded]))
    assert gd < 0
    assert float(fc) - efc > float(lin.cost) + lin.cost_bound + 1e-4 * gd


def test_a_rejected_step_is_found(P):
    cfg = _cfg(P, "reject_W4")
    case = R.get_case("reject_W4", cfg)
    assert case["reject_scale"] in R.REJECT_SCALES


def test_forward_bound_list():
    assert len(R.FWD_UNBOUNDED) * 8 <= len(NAMES) and set(R.FWD_UNBOUNDED) <= set(NAMES)


@pytest.mark.parametrize("name", ["base_W4", "two_frames_W10"])
def test_long_double_and_mpmath_agree(P, name):
    cfg, pb, X, feat, lin, st = _at_x0(P, name)
    mp = R.linearise(pb, X, feat, route="mp")
    for k, E in (("H", lin.EH), ("g", lin.Eg), ("Hpl", lin.EHpl), ("Hll", lin.EHll), ("gl", lin.Egl)):
        a, b = D._as_ld(getattr(mp, k)), getattr(lin, k)
        d = np.abs(D._f64(a - b))
        assert np.all(d <= 1e-3 * E), (name, k, float(np.max(d / np.where(E > 0, E, 1.0))))
    assert abs(float(D._as_ld(np.array([mp.cost]))[0] - lin.cost)) <= 1e-3 * lin.cost_bound
    st2 = R.gn_system(pb, mp, R.scaling(pb, mp))
    assert np.all(np.abs(D._f64(st2.y - st.y)) <= 1e-3 * st.y_bound)


def test_zz_report_worst_ratios():
    print("WORST float64 numpy error / bound:", " ".join("%s=%.3g" % kv for kv in sorted(_worst.items())))
    if _steps:
        v = np.array(_steps["step_bar_rel"])
        print("float64 numpy step difference / max|step| (the measurement of (c)): min %.3g median %.3g max %.3g" % (v.min(), np.median(v), v.max()))
