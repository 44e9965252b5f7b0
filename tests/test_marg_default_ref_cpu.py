"""tests/marg_default_ref.py against itself, without a GPU: every case of tests/test_gpu_marg_default.py reaches the edge it is named for (on the
reference alone), the mpmath and long-double routes agree, and float64 numpy on the same inputs lies inside every bound.

Worst error / bound of the float64 numpy evaluation (np_eval: numpy.linalg.eigh pseudo-inverse, numpy.linalg.cholesky for c0) over all cases:
A_r 0.62, b_r 0.027, prior_H 0.62, prior_r 0.027, c0 0.00053 against the reference and 0.0039 against c0_self (bounds: 1; per kind of case in DESIGN.md section 5a).

c0 is compared twice.  Against the reference's c0 where the definition bounds it (`c0_bounded`): UNBOUNDED_C0 below lists the cases where it does
not -- the new prior is singular to within its own error, because there is no prior at all (the gauge directions) or because fewer than three
marginalised landmarks see the newest pose.  And, in every case, against c0 formed in mpmath from the RETURNED prior_H and prior_r
(marg_default_ref.c0_self: the kernel's Cholesky solve of the lifted matrix held to its own forward error, whatever the error of H), which covers the
cases of UNBOUNDED_C0 as well -- except the six first marginalisations without a prior, marg_default_ref.C0_UNDETERMINED, where the lifted matrix is
not positive definite to within the solve's backward error (reason there).  test_c0_lists pins both lists by name."""
import numpy as np
import pytest

import marg_default_ref as D

L = np.longdouble


def _cfg(P, name):
    return P.canonical_config(**D.cfg_kwargs(name))


NAMES = sorted(D.CASES)
LIVE = [n for n in NAMES if n not in D.NOOP]


def test_case_list_covers_the_sizes_and_kinds():
    Ws = {D.CASES[n][0] for n in NAMES}
    assert Ws == {4, 10, 12, 20}
    assert {D.CASES["F0_%d_W4" % f][1]["F0"] for f in D.F0_LIST} == set(D.F0_LIST) == {0, 1, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130}
    for kind in D.KINDS:
        assert kind + "_W4" in D.CASES and kind + "_W10" in D.CASES


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge(P, name):
    """on the reference alone: the landmarks under the cut, the route of the pseudo-inverse, the structure the case is named for"""
    cfg = _cfg(P, name)
    case, r = D.get_case(name, cfg), D.get_ref(name, cfg)
    W, kw = D.CASES[name]
    st = case["st"]
    if name in D.NOOP:
        assert r.noop and st["marginalization_flag"] == 1
        assert r.has_prior == int(st["prior"] is not None)
        return
    assert not r.noop and r.bounded, (r.rho_mm, r.n_dropped, r.zero_rows)
    # the list: exactly F0 landmarks, in an order that is not slot order, beside the four kinds that must be ignored
    if not r.second_new:
        assert len(r.list) == kw.get("F0", D.DEFAULTS["F0"])
        if len(r.list) > 3:
            assert r.list != sorted(r.list)
        nobs = [int(st["lm_nobs"][s]) for s in r.list]
        if len(nobs) >= 15 and not kw.get("flat"):
            assert min(nobs) == 2 and max(nobs) == (W if kw.get("blind") else W + 1)
        ignored = [s for s in st["lm_order"] if s not in r.list]
        assert any(st["lm_dyn"][s] for s in ignored) and any(st["lm_nobs"][s] == 1 for s in ignored)
        assert any(0 < st["lm_start"][s] < W - 2 for s in ignored) or W <= 4
        assert any(st["lm_start"][s] >= W - 2 for s in ignored)
    assert st["ring_base"] != 0 and list(st["pre_idx"]) != list(range(W + 1))
    # landmarks at the cut: none within 1e-3 relative of it, and none whose own error could move it across
    d, de = np.array(r.d), np.array(r.d_err)
    assert int((d <= D.CUT).sum()) == D.N_FLAT[name], (d[d <= 1.0], D.N_FLAT[name])
    assert np.all(np.abs(d - D.CUT) > 1e-3 * D.CUT) and np.all(np.abs(d - D.CUT) > 10 * de)
    if D.N_FLAT[name]:
        assert d[d <= D.CUT].max() <= 1e-20 and d[d > D.CUT].min() >= 1.0
    # the m-block: direct inverse (everything >= 1e-5) or the eigen route (exact zeros dropped), nothing in between
    if name in D.EIGEN_ROUTE:
        assert r.n_dropped == 9 and list(r.zero_rows) == list(range(6, 15)) and abs(r.lam_drop_max) <= 1e-30
        assert r.lam_kept_min >= 1e-5
        assert not r.present[W]                                    # no factor touches the new speed-bias
    else:
        assert r.n_dropped == 0 and r.lam_kept_min >= 1e-5
    assert r.md == (6 if r.second_new else 15)
    if kw.get("moved"):
        assert r.w_min < -0.9 and np.abs(r.dx).max() > 1e-3      # a pose whose q0^-1 q has a negative scalar part, and a state off x0
    if kw.get("outlier"):
        assert min(r.weights) < 0.05
    if kw.get("blind"):
        assert not r.present[W - 1] and not D._f64(r.A)[r.md + 6 * (W - 1):r.md + 6 * W].any()
    if kw.get("long_dt"):
        assert r.sum_dt >= 10.0 and not r.imu_used
    if kw.get("prior", "full") == "absent":
        pr = st["prior"]
        assert not pr["present"][1] and not pr["H"][6:12].any() and not pr["H"][:, 6:12].any() and not pr["r"][6:12].any()
        assert not pr["present"][W + 1] and bool(pr["present"][W - 1]) == r.second_new
    if st["prior"] is not None:
        assert np.array_equal(st["prior"]["H"], st["prior"]["H"].T) and np.linalg.eigvalsh(st["prior"]["H"])[0] >= -1e-9 * np.abs(st["prior"]["H"]).max()
    if W == 20 and not r.second_new:
        assert max(int(st["lm_nobs"][s]) for s in r.list) > 17       # the second trip of the sixteen-lane loop


def test_the_two_routes_agree(P):
    """the same case through 40-digit mpmath and through long double: equal to 1e-17 of each entry's sum of absolute terms"""
    name = "F0_17_W4"
    cfg = _cfg(P, name)
    case = D.get_case(name, cfg)
    a, b = D.reference(case, cfg, route="mp"), D.reference(case, cfg, route="ld")
    assert a.route == "mp" and b.route == "ld"
    eA = np.abs((a.A - b.A).astype(np.float64))
    assert np.all(eA <= 1e-17 * a.absA + 1e-300), float(np.max(eA / (a.absA + 1e-300)))
    eb = np.abs((a.b - b.b).astype(np.float64))
    assert np.all(eb <= 1e-17 * a.absb + 1e-300)
    # A_r and b_r inherit the block's conditioning: both routes within 1e-6 of the tightest bound
    assert np.all(np.abs((a.Ar - b.Ar).astype(np.float64)) <= 1e-6 * a.Ar_bound + 1e-300)
    assert np.all(np.abs((a.br - b.br).astype(np.float64)) <= 1e-6 * a.br_bound + 1e-300)
    assert abs(float(a.c0 - b.c0)) <= 1e-6 * a.c0_bound
    assert D.get_ref(name, cfg).route == "mp" and D.get_ref("F0_63_W4", _cfg(P, "F0_63_W4")).route == "ld"


def test_the_two_routes_agree_at_w10(P):
    """a W = 10 case (mq = 91, F0 = 17), which the suite runs in long double, once through mpmath as well"""
    name = "F0_17_W10"
    cfg = _cfg(P, name)
    b = D.get_ref(name, cfg)
    a = D.reference(D.get_case(name, cfg), cfg, route="mp")
    assert a.route == "mp" and b.route == "ld"
    assert np.all(np.abs((a.A - b.A).astype(np.float64)) <= 1e-17 * a.absA + 1e-300)
    assert np.all(np.abs((a.b - b.b).astype(np.float64)) <= 1e-17 * a.absb + 1e-300)
    assert np.all(np.abs((a.Ar - b.Ar).astype(np.float64)) <= 1e-6 * a.Ar_bound + 1e-300)
    assert np.all(np.abs((a.br - b.br).astype(np.float64)) <= 1e-6 * a.br_bound + 1e-300)
    assert abs(float(a.c0 - b.c0)) <= 1e-6 * a.c0_bound


_worst = {}


@pytest.mark.parametrize("name", LIVE)
def test_float64_numpy_is_inside_every_bound(P, name):
    cfg = _cfg(P, name)
    r = D.get_ref(name, cfg)
    Ar, br, H, c0 = D.np_eval(r)
    q = D.ratios(r, H, br, c0, Ar=Ar, br=br)
    cs = D.c0_self_ratio(name, H, br, c0)
    if cs is not None:
        q["c0_self"] = cs
    for k, v in q.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    print("MEASURED numpy", name, " ".join("%s=%.3g" % kv for kv in sorted(q.items())))
    assert max(q.values()) <= 1.0, q
    assert np.array_equal(H, H.T)


def test_the_bounds_notice_a_wrong_term(P):
    """The bounds are tight enough to mean something: float64 numpy with one of the mistakes the GPU test exists for lies far outside them --
    the last landmark of the list dropped (a lost tail), the extrinsic columns mapped one off, the prior's pose delta taken at the wrong sign of
    q0^-1 q."""
    import copy
    name = "moved_W4"
    cfg = _cfg(P, name)
    case, r = D.get_case(name, cfg), D.get_ref(name, cfg)
    md, W = r.md, r.W
    # a lost tail
    c2 = copy.deepcopy(case)
    c2["st"]["lm_dyn"][r.list[-1]] = 1
    r2 = D.reference(c2, cfg)
    assert len(r2.list) == len(r.list) - 1
    Ar, br, H, c0 = D.np_eval(r2)
    q = D.ratios(r, H, br, c0, Ar=Ar, br=br)
    assert q["H"] > 1e3 and q["r"] > 1e3, q
    # the extrinsic block one column off
    rE = md + 6 * W + 9
    perm = np.arange(r.mq)
    perm[rE:rE + 6] = np.roll(perm[rE:rE + 6], 1)
    A, b = D._f64(r.A), D._f64(r.b)
    Ar, br, H, c0 = D.np_eval(r, A=A[np.ix_(perm, perm)], b=b[perm])
    q = D.ratios(r, H, br, c0, Ar=Ar, br=br)
    assert q["H"] > 1e3 and q["r"] > 1e3, q
    # the rotation part of pose 2's delta with the wrong sign (its q0^-1 q has a negative scalar part)
    pr = case["st"]["prior"]
    a = np.arange(6 * 2 + 3, 6 * 2 + 6)
    b2 = b.copy()
    b2[r.prior_idx] -= 2.0 * pr["H"][:, a] @ r.dx[a]
    Ar, br, H, c0 = D.np_eval(r, b=b2)
    q = D.ratios(r, H, br, c0, Ar=Ar, br=br)
    assert q["r"] > 1e3 and q["H"] <= 1.0, q


UNBOUNDED_C0 = ["F0_1_W4", "F0_4_W4", "F0_5_W4", "flat1_W10", "flat1_W4", "long_dt_W10", "long_dt_W4", "moved_absent_W10", "moved_absent_W4",
                "no_imu_W10", "no_imu_W4", "no_prior_W10", "no_prior_W4", "wide_W20_moved"]


def test_c0_lists(P):
    """the cases whose c0 the reference cannot bound, and the cases whose c0 is not determined even by the returned prior, by name"""
    refs = {n: D.get_ref(n, _cfg(P, n)) for n in LIVE}
    assert sorted(n for n in LIVE if not refs[n].c0_bounded) == UNBOUNDED_C0
    for n in UNBOUNDED_C0:      # the reason: no prior, or too few landmarks on the newest pose
        W, kw = D.CASES[n]
        assert kw.get("prior", "full") is None or kw.get("F0", D.DEFAULTS["F0"]) <= 5, n
    # where it is bounded the bound means something: below 1e-3 of c0
    for n in LIVE:
        if refs[n].c0_bounded and float(refs[n].c0) > 0:
            assert refs[n].c0_bound <= 1e-3 * float(refs[n].c0), (n, refs[n].c0_bound, float(refs[n].c0))
    # the second comparison: undetermined exactly for the first marginalisations without a prior
    und = []
    for n in LIVE:
        Ar, br, H, c0 = D.np_eval(refs[n])
        cs, bound, rho, pd = D.c0_self(H, br)
        if not (pd and rho < 0.5):
            und.append(n)
        elif cs > 0:
            assert bound <= 1e-6 * cs, (n, bound, cs)
    assert set(und) <= set(D.C0_UNDETERMINED) and set(D.C0_UNDETERMINED) <= set(UNBOUNDED_C0), und
    assert all(D.CASES[n][1].get("prior", "full") is None for n in D.C0_UNDETERMINED)
    assert sorted(D.C0_UNDETERMINED) == sorted(n for n in LIVE if D.CASES[n][1].get("prior", "full") is None and not refs[n].second_new)


def test_zz_report_worst_ratios():
    print("WORST numpy error / bound:", " ".join("%s=%.3g" % kv for kv in sorted(_worst.items())))
