"""The phased solver launch by launch -- ps_setup, ps_eval / ps_evalf, ps_asm_a, ps_asm_b_schur, ps_serial_kernel_512 / ps_serial_big_kernel, ps_ls,
ps_final -- against its definition (tests/solve_ref.py: Ceres' trust-region minimiser with the dogleg strategy, factors from factor_ref, sums, the
full unreduced solve and the dogleg in extended precision, bounds derived there) on staged window states: vio_debug_solve_set writes a generated
state into a real handle, vio_debug_solve_run launches the solver's kernels up to a chosen phase, vio_debug_solve_get reads every intermediate by name.

Per case and handle (default, VIO_FUSE=1, VIO_EVAL_RPT=1, VIO_EVAL_RPT=2):
  (a) after the first evaluation, assembly and Schur launch: what ps_setup decided (F, Fa, nres, the variable landmarks in solver order, which blocks
      are open, constrained), the staged point (bit for bit; quaternions within 8 eps), the cost, H, g over the open parameters, Hpl, Hll, gl, the
      Jacobi scaling, and U (the landmark part of the Schur complement) against the linearisation of the definition at that point, entrywise;
  (b) after ps_serial: the Gauss-Newton step put into the reference's full regularised system (residual bound of a backward-stable solve) and,
      where C N eps kappa <= 1e-3, against the reference's solution; the trust-region diagonal;
  (c) at three radii, one per dogleg branch: the step, dogleg_norm, model_change, alpha, and the candidate Plus(x0, step) through factor_ref.pose_plus;
  (d) after the next evaluation: ccost against the definition's cost at the candidate the device formed, the accept / reject decision, the new
      radius, and the window bit for bit (the candidate when accepted, x0 when rejected);
  (e) bounds-constrained: x0 projected onto the box, the accepted candidate = Plus(x0, a delta), 0 < a <= 1, inside the box and satisfying the
      Armijo condition evaluated by the definition;
  (f) the whole solve (slots < 0): cost at the returned point <= cost at x0 by the definition; all slots through the harness leave the same bits.
The default and fused handles are also compared with each other within (a); two sequences staged beside an idle one equal their single runs bit
for bit; malformed tables are refused and nothing runs.  From the second slot on ps_asm_b_schur forms S itself: Sc against the reference's Schur
complement and the second Gauss-Newton step at the accepted candidate (test_second_slot_forms_s_and_solves_it).  A fallback handle
(VIO_SOLVE_MODE=0) accepts the whole solve only; with max_iterations = 1 its window and depths equal the definition's candidate after the gauge fix.

Worst device error / bound over all cases and handles, measured on an MI355X (test_zz_report_worst_ratios prints them): cost
0.0039, H 0.038, g 0.023, Hpl 0.035, Hll 0.020, gl 0.025, sp 0.015, sl 0.017, U 0.0080, D 0.065, Gauss-Newton residual 0.0058 and forward error
0.0013, step 0.0013, dogleg_norm 0.0053, alpha 3.4e-4, model_change 7.5e-4, Xc 0.043, ccost 0.0058, final cost 0.0025; second slot: S 0.043,
Gauss-Newton residual 0.014, forward error 1.2e-4, D 0.065; fallback handle: P 1.3e-7, R 2.1e-7, V 1.8e-7, bias 2.3e-6, depth 8.2e-7.  The whole
file takes 42 s, references included."""
import numpy as np
import pytest

import marg_default_ref as D
import solve_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("VIO_FUSE", "VIO_EVAL_RPT", "VIO_SOLVE_MODE", "VIO_GROUP_SEQS", "VIO_EXTRA_SLOTS", "VIO_LINE_SEARCH", "VIO_MARG_SPLIT")
ENV = dict(default={}, fuse=dict(VIO_FUSE="1"), rpt1=dict(VIO_EVAL_RPT="1"), rpt2=dict(VIO_EVAL_RPT="2"), fallback=dict(VIO_SOLVE_MODE="0"))
PHASED = ("default", "fuse", "rpt1", "rpt2")
_handles, _worst = {}, {}
EPS = D.EPS
L = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for b in _handles.values():
        b.close()
    _handles.clear()


def handle(P, monkeypatch, name, kind, S=1, **extra):
    ck = dict(R.cfg_kwargs(name), **extra)
    key = (tuple(sorted(ck.items())), kind, S)
    if key not in _handles:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in ENV[kind].items():
            monkeypatch.setenv(k, v)
        _handles[key] = P.VioBatch(P.canonical_config(**ck), S)
    return _handles[key]


def cfg_of(P, name):
    return P.canonical_config(**R.cfg_kwargs(name))


def stage(P, b, name, seq=0):
    cfg = cfg_of(P, name)
    b.solve_stage_set(seq, D.pad_tables(R.get_case(name, cfg)["st"], b.capacity()["landmarks"]))


def note(q, name, tag):
    print("MEASURED device", name, tag, " ".join("%s=%.3g" % kv for kv in sorted(q.items())))
    for k, v in q.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    assert max(q.values()) <= 1.0, (name, tag, {k: v for k, v in q.items() if v > 1.0})


def same_point(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("pose", "sb", "ex")) and a["td"] == b["td"]


def fused_expected(pb, kind):
    Cc = R.PS_FUSE_CAP - pb.W
    return int(kind == "fuse" and not pb.vext and pb.W <= 10 and (pb.nres + Cc - 1) // Cc <= 12 and pb.use_imu)


def check_setup(pb, o, kind, X0, feat0):
    """what ps_setup decided, and the staged point"""
    assert (o["F"], o["Fa"], o["nres"]) == (pb.F, pb.Fa, pb.nres), (o["F"], o["Fa"], o["nres"], pb.F, pb.Fa, pb.nres)
    assert (o["ex_active"], o["td_active"], o["vext"], o["constrained"]) == (int(pb.ex_active), int(pb.td_active), int(pb.vext), int(pb.constrained))
    assert o["fused"] == fused_expected(pb, kind)
    assert list(o["var_slots"]) == pb.alist
    X = o["X"]
    assert np.array_equal(X["pose"][:, :3], X0["pose"][:, :3]) and np.array_equal(X["sb"], X0["sb"]) and np.array_equal(X["ex"][:3], X0["ex"][:3])
    assert X["td"] == X0["td"]
    assert np.abs(X["pose"][:, 3:] - X0["pose"][:, 3:]).max() <= 8 * EPS and np.abs(X["ex"][3:] - X0["ex"][3:]).max() <= 8 * EPS
    assert np.array_equal(o["feat"], feat0), np.flatnonzero(o["feat"] != feat0)


def check_linearisation(pb, o, lin, st):
    """(a): dict of error / bound"""
    act, na, W1, P = pb.act, len(pb.act), pb.W1, pb.P
    ix = np.ix_(act, act)
    q = dict(cost=R.ratio(o["cost"], lin.cost, lin.cost_bound), H=R.ratio(o["H"][ix], lin.H[ix], lin.EH[ix]), g=R.ratio(o["g"][act], lin.g[act], lin.Eg[act]))
    assert np.array_equal(o["H"], o["H"].T)
    cols = np.r_[np.arange(6 * W1), (pb.oE + np.arange(7)) if pb.vext else np.zeros(0, int)].astype(int)
    if pb.Fa:
        q["Hpl"] = R.ratio(o["Hpl"][:, cols], lin.Hpl[:, cols], lin.EHpl[:, cols])
        q["Hll"] = R.ratio(o["Hll"], lin.Hll, lin.EHll)
        q["gl"] = R.ratio(o["gl"], lin.gl, lin.Egl)
    # Jacobi scaling: 0 for constant parameters, 1 / (1 + sqrt(H_aa)) within its first-order bound
    sp = o["sp"]
    const = np.setdiff1d(np.arange(P), act)
    assert not sp[const].any() and (sp[act] > 0).all()
    q["sp"] = R.ratio(sp[act], st.s[:na], D._f64(st.s[:na]) * st.q[:na])
    # U in the tiles the landmark rows touch (first slot: the column scaling is still to be fixed)
    if pb.Fa:
        U, EU, _ = R.schur_u(pb, lin, st.s)
        LW = o["Sc"].shape[0]
        tile_on = [cb for cb in range(LW // 16) if 16 * cb < 6 * W1 or (pb.vext and 16 * cb + 15 >= 15 * W1 and 16 * cb < 15 * W1 + 7)]
        rows = np.array([a for cb in tile_on for a in range(16 * cb, 16 * cb + 16)])
        Sd = o["Sc"][np.ix_(rows, rows)]
        low = (rows[:, None] // 16 > rows[None, :] // 16) | ((rows[:, None] // 16 == rows[None, :] // 16))
        Ur, Er = np.zeros((len(rows), len(rows)), L), np.zeros((len(rows), len(rows)))
        inP = rows < P
        Ur[np.ix_(inP, inP)] = U[np.ix_(rows[inP], rows[inP])]
        Er[np.ix_(inP, inP)] = EU[np.ix_(rows[inP], rows[inP])]
        q["U"] = R.ratio(Sd[low], Ur[low], Er[low])
    return q


def check_gn(pb, o, st):
    """(b): dict of error / bound"""
    act, na = pb.act, len(pb.act)
    y = np.concatenate([-o["gnp"][act] / o["dgp"][act], -o["gnl"] / o["dgl"]])
    res = np.abs(D._f64(st.M @ y.astype(L) - st.gs))
    q = dict(gn_residual=float(np.max(res / (st.res_bound_of(np.abs(y)) + 4 * EPS * np.abs(y) * st.dd * st.dd))))   # (+ the two roundings of - gn / D)
    if st.fwd_bounded:
        q["gn_forward"] = R.ratio(y, st.y, st.y_bound + 4 * EPS * np.abs(D._f64(st.y)))
    dgv = np.concatenate([o["dgp"][act], o["dgl"]])
    Dg = D._f64(st.Dg)
    q["D"] = R.ratio(dgv, st.Dg, 0.5 * np.diag(st.EM) / Dg + 3 * EPS * Dg)
    if pb.Fa:
        q["sl"] = R.ratio(o["sl"], st.s[na:], D._f64(st.s[na:]) * st.q[na:])
    return q


def check_step(pb, o, st, X, feat, radius, branch):
    """(c): dict of error / bound"""
    act, na = pb.act, len(pb.act)
    bar, ref = R.bars(pb, X, feat, st, radius)
    assert ref["branch"] == branch
    z = np.concatenate([o["stp"][act] * o["dgp"][act], o["stl"] * o["dgl"]])
    q = dict(step=R.ratio(z, ref["z"], bar["z"] + 4 * EPS * np.abs(z)))
    if branch == "cauchy":
        assert o["dogleg_norm"] == radius
    else:
        q["dogleg_norm"] = R.ratio(o["dogleg_norm"], ref["norm"], bar["norm"])
    q["model_change"] = R.ratio(o["model_change"], ref["model_change"], bar["model_change"])
    if branch != "gn":
        q["alpha"] = R.ratio(o["alpha"], ref["alpha"], bar["alpha"])
    # the candidate: Plus(x0, the step the device returned)
    delta, dl = o["sp"] * o["stp"], o["sl"] * o["stl"]
    Xc, cf, sc = R.plus(pb, X, feat, delta, dl)
    assert np.array_equal(o["Xc"]["sb"], Xc["sb"]) and o["Xc"]["td"] == Xc["td"]
    assert np.array_equal(o["cfeat"], cf), np.flatnonzero(o["cfeat"] != cf)
    q["Xc"] = max(R.ratio(o["Xc"]["pose"], Xc["pose"], D.KF * EPS * sc["pose"]), R.ratio(o["Xc"]["ex"], Xc["ex"], D.KF * EPS * sc["ex"]))
    return q, ref


def run_case(P, monkeypatch, name, kind, full=True):
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    b = handle(P, monkeypatch, name, kind)
    X0, feat0 = pb.x0()
    # ---- (a)
    stage(P, b, name)
    b.solve_stage_run(0, "schur")
    o = b.solve_stage_get(0)
    assert o["stage"] == "asm" and b.status(0).code >= 0
    check_setup(pb, o, kind, X0, feat0)
    X, feat = o["X"], o["feat"]
    lin, st = R.lin_at(name, cfg, X, feat)
    note(check_linearisation(pb, o, lin, st), name, kind + "/a")
    out = dict(a=o)
    if not full:
        return out
    # ---- (b), (c)
    rr, _, _ = R.radii(st)
    first = True
    for branch, radius in rr.items():
        if radius is None:
            continue
        stage(P, b, name)
        b.solve_stage_run(0, "serial", radius0=0.0 if radius == R.RADIUS0 else radius)
        o = b.solve_stage_get(0)
        assert o["stage"] == "eval_c" and o["iter"] == 1 and o["radius"] == radius
        if first:
            note(check_gn(pb, o, st), name, kind + "/b")
            first = False
        q, ref = check_step(pb, o, st, X, feat, radius, branch)
        note(q, name, kind + "/c-" + branch)
        if pb.constrained:
            continue
        # ---- (d): the next evaluation
        stage(P, b, name)
        b.solve_stage_run(1, "asm_a", radius0=0.0 if radius == R.RADIUS0 else radius)
        o2 = b.solve_stage_get(0)
        assert same_point(o2["Xc"], o["Xc"]) and np.array_equal(o2["cfeat"], o["cfeat"]) and o2["model_change"] == o["model_change"]
        fc, efc = R.cost(pb, o2["Xc"], o2["cfeat"])
        note(dict(ccost=R.ratio(o2["ccost"], fc, efc)), name, kind + "/d-" + branch)
        ok, new_radius, rho = R.step_control(lin.cost, fc, ref["model_change"], radius, o["dogleg_norm"])
        if ok:
            assert o2["stage"] == "asm" and same_point(o2["X"], o["Xc"]) and np.array_equal(o2["feat"], o["cfeat"]), (name, branch, rho, o2["stage"])
            assert abs(o2["cost"] - o2["ccost"]) <= 64 * EPS * abs(o2["cost"])      # (ps_accept adds the partial costs in tree order, the harness in index order)
        else:
            assert o2["stage"] == "step" and same_point(o2["X"], X) and np.array_equal(o2["feat"], feat), (name, branch, rho, o2["stage"])
            assert o2["cost"] == out["a"]["cost"]
        assert o2["radius"] == new_radius, (name, branch, rho, o2["radius"], new_radius)
        out["d-" + branch] = o2
    return out


SMALL = sorted(n for n in R.CASES if not n.startswith("nres"))
NRES = sorted(n for n in R.CASES if n.startswith("nres"))


def kinds_of(name):
    if name.startswith("nres"):
        n = int(name[4:7])
        return {251: ["fuse"], 252: ["fuse"], 253: ["fuse"], 255: ["rpt1", "fuse"], 256: ["rpt1", "fuse"], 257: ["rpt1", "fuse"]}.get(n, ["default", "rpt2"])
    return ["default", "fuse", "rpt1"]


@pytest.mark.parametrize("name", SMALL + NRES)
def test_against_the_definition(P, monkeypatch, name):
    outs = {}
    for i, kind in enumerate(kinds_of(name)):
        outs[kind] = run_case(P, monkeypatch, name, kind, full=(i == 0 or not name.startswith("nres")))
    # the handles against each other, within (a)
    kinds = list(outs)
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    a0 = outs[kinds[0]]["a"]
    lin, st = R.lin_at(name, cfg, a0["X"], a0["feat"])
    ix = np.ix_(pb.act, pb.act)
    for kind in kinds[1:]:
        a1 = outs[kind]["a"]
        assert same_point(a0["X"], a1["X"])
        q = dict(H=R.ratio(a1["H"][ix], a0["H"][ix], 2 * lin.EH[ix]), g=R.ratio(a1["g"][pb.act], a0["g"][pb.act], 2 * lin.Eg[pb.act]))
        if pb.Fa:
            q.update(Hpl=R.ratio(a1["Hpl"], a0["Hpl"], 2 * lin.EHpl), Hll=R.ratio(a1["Hll"], a0["Hll"], 2 * lin.EHll), gl=R.ratio(a1["gl"], a0["gl"], 2 * lin.Egl))
        assert max(q.values()) <= 1.0, (name, kinds[0], kind, q)


SECOND = [("base_W4", "default"), ("base_W4", "fuse"), ("base_W10", "default"), ("base_W10", "fuse"), ("big_W11", "default"), ("absent_W10", "default"),
          ("no_imu_W4", "default"), ("ex_td_fast_W4", "default"), ("ex_td_slow_W4", "default"), ("flat_W4", "default"), ("Fa3_W4", "default"),
          ("Fa0_W4", "default"), ("long_dt_W4", "rpt1"), ("nres257_W4", "rpt1")]


@pytest.mark.parametrize("name,kind", SECOND)
def test_second_slot_forms_s_and_solves_it(P, monkeypatch, name, kind):
    """(b) beyond the first slot: once the column scaling is fixed, ps_asm_b_schur forms S = Sp (H - U) Sp + mu D^2 itself (clamp, unit diagonal of
    constant and padding parameters) and ps_serial only factorises it.  At the accepted candidate of the full step: Sc against the reference's
    Schur complement entrywise, H, g and the landmark rows of the new point, and the second Gauss-Newton step by residual (and forward error)
    in the reference's system with the FIRST linearisation's scaling."""
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    b = handle(P, monkeypatch, name, kind)
    stage(P, b, name)
    b.solve_stage_run(0, "schur")
    o0 = b.solve_stage_get(0)
    _, st0 = R.lin_at(name, cfg, o0["X"], o0["feat"])
    stage(P, b, name)
    b.solve_stage_run(1, "schur")
    o1 = b.solve_stage_get(0)
    assert o1["stage"] == "asm" and o1["iter"] == 1 and not same_point(o1["X"], o0["X"]), "the full step of this case is accepted"
    assert np.array_equal(o1["sp"], o0["sp"]) and o1["mu"] == R.MU0
    lin1, _ = R.lin_at(name, cfg, o1["X"], o1["feat"])
    st1 = R.gn_system(pb, lin1, st0.s, mu=o1["mu"], q=st0.q)
    act, na, Pn = pb.act, len(pb.act), pb.P
    ix = np.ix_(act, act)
    q = dict(H=R.ratio(o1["H"][ix], lin1.H[ix], lin1.EH[ix]), g=R.ratio(o1["g"][act], lin1.g[act], lin1.Eg[act]))
    if pb.Fa:
        cols = np.r_[np.arange(6 * pb.W1), (pb.oE + np.arange(7)) if pb.vext else np.zeros(0, int)].astype(int)
        q.update(Hpl=R.ratio(o1["Hpl"][:, cols], lin1.Hpl[:, cols], lin1.EHpl[:, cols]), Hll=R.ratio(o1["Hll"], lin1.Hll, lin1.EHll),
                 gl=R.ratio(o1["gl"], lin1.gl, lin1.Egl))
    S, ES = R.schur_s(st1)
    LW = o1["Sc"].shape[0]
    Sr, Er = np.eye(LW, dtype=L), np.zeros((LW, LW))
    Sr[ix], Er[ix] = S, ES
    idx = np.arange(LW)
    low = idx[:, None] // 16 >= idx[None, :] // 16
    q["S"] = R.ratio(o1["Sc"][low], Sr[low], Er[low])
    stage(P, b, name)
    b.solve_stage_run(1, "serial")
    o2 = b.solve_stage_get(0)
    assert o2["stage"] == "eval_c" and o2["iter"] == 2 and same_point(o2["X"], o1["X"])
    q2 = check_gn(pb, o2, st1)
    q2.pop("sl", None)
    q.update({k + "_2": v for k, v in q2.items()})
    note(q, name, kind + "/second")


@pytest.mark.parametrize("name,kind", [("bounded_W4", "default"), ("bounded_W4", "fuse"), ("bounded_reject_W4", "default"), ("bounded_reject_W4", "rpt1")])
def test_constrained_solve(P, monkeypatch, name, kind):
    """(e); bounded_W4's projected full step satisfies the Armijo condition (a = 1), bounded_reject_W4's does not (the CPU test asserts it): the
    line search has to shorten it"""
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    assert pb.constrained
    b = handle(P, monkeypatch, name, kind)
    X0, feat0 = pb.x0()
    stage(P, b, name)
    b.solve_stage_run(0, "ls")
    o = b.solve_stage_get(0)
    assert o["constrained"] == 1 and o["stage"] == "eval_c"
    assert np.array_equal(o["feat"], feat0) and all(feat0[pb.var[q]] <= pb.ub for q in pb.bounded)
    if name == "bounded_W4":
        assert feat0[pb.var[pb.bounded[0]]] == pb.ub          # staged beyond the bound, projected at x0
    X, feat = o["X"], o["feat"]
    lin, st = R.lin_at(name, cfg, X, feat)
    # the candidate is Plus(x0, a delta) for one a in (0, 1]: a from the largest entry of the landmark step, checked on every block
    delta, dl = o["sp"] * o["stp"], o["sl"] * o["stl"]
    free = [a for a in range(pb.Fa) if a not in pb.bounded]
    k = free[int(np.argmax(np.abs(dl[free])))]
    a = float((o["cfeat"][pb.var[k]] - feat[pb.var[k]]) / dl[k])
    assert 0.0 < a <= 1.0 + 4 * EPS, a
    assert (a < 0.999) == (name == "bounded_reject_W4"), (name, a)
    Xc, cf, sc = R.plus(pb, X, feat, min(a, 1.0) * delta, min(a, 1.0) * dl)
    tol = 16 * EPS / max(a, 1e-3)
    assert np.abs(o["Xc"]["sb"] - Xc["sb"]).max() <= tol * (np.abs(X["sb"]).max() + np.abs(delta).max())
    assert np.abs(o["Xc"]["pose"] - Xc["pose"]).max() <= tol * (np.abs(X["pose"]).max() + np.abs(delta).max()) + D.KF * EPS * sc["pose"].max()
    assert np.abs(o["cfeat"] - cf).max() <= tol * (np.abs(feat).max() + np.abs(dl).max())
    assert all(o["cfeat"][pb.var[q]] <= pb.ub for q in pb.bounded)
    # Armijo, evaluated by the definition at the device's candidate
    fc, efc = R.cost(pb, o["Xc"], o["cfeat"])
    gd = float(D._f64(lin.g[pb.act]) @ delta[pb.act] + D._f64(lin.gl) @ dl)
    assert gd < 0
    assert float(fc) - efc <= float(lin.cost) + lin.cost_bound + 1e-4 * a * gd * (1 - 1e-6), (float(fc), float(lin.cost), a, gd)


WHOLE = [(n, k) for n in ("base_W4", "base_W10", "big_W11", "reject_W4", "bounded_W4", "ex_td_fast_W4") for k in ("default", "fuse", "rpt1")] + [("base_W4", "rpt2")]


@pytest.mark.parametrize("name,kind", WHOLE)
def test_whole_solve(P, monkeypatch, name, kind):
    """(f)"""
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    b = handle(P, monkeypatch, name, kind)
    stage(P, b, name)
    b.solve_stage_run(-1)
    w = b.solve_stage_get(0)
    assert w["stage"] == "idle" and b.status(0).code >= 0
    X0, feat0 = pb.x0()
    f0, e0 = R.cost(pb, X0, feat0)
    f1, e1 = R.cost(pb, w["X"], w["feat"])
    assert float(f1) - e1 <= float(f0) + e0, (float(f0), float(f1))
    note(dict(final_cost=R.ratio(w["cost"], f1, e1)), name, kind + "/f")
    slots = int(cfg.max_iterations) + 2
    stage(P, b, name)
    b.solve_stage_run(slots, "none")
    s = b.solve_stage_get(0)
    assert s["stage"] == "done"
    assert same_point(s["X"], w["X"]) and np.array_equal(s["feat"], w["feat"]) and s["cost"] == w["cost"]
    assert (s["iter"], s["iters_done"], s["radius"], s["mu"]) == (w["iter"], w["iters_done"], w["radius"], w["mu"])
    # slot by slot: each run repeats the previous one's state and goes one slot further; the costs never rise
    prev = None
    for k in range(slots + 1):
        stage(P, b, name)
        b.solve_stage_run(k, "none")
        o = b.solve_stage_get(0)
        if k >= 2:                                   # (the first slot evaluates x0: there is no cost before it)
            assert o["cost"] <= prev
        prev = o["cost"]
    assert same_point(o["X"], w["X"]) and o["cost"] == w["cost"]


def test_fallback_handle_runs_the_whole_solve_only(P, monkeypatch):
    name = "base_W4"
    b = handle(P, monkeypatch, name, "fallback")
    stage(P, b, name)
    with pytest.raises(P.VioError):
        b.solve_stage_run(0, "schur")
    with pytest.raises(P.VioError):
        b.solve_stage_get(0)
    b.solve_stage_run(-1)
    assert b.status(0).code >= 0


def _rotm(qwxyz):
    w, x, y, z = qwxyz
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("name", ["base_W4", "no_prior_W4", "base_W10"])
def test_fallback_handle_returns_the_definitions_candidate(P, monkeypatch, name):
    """(f) on the persistent kernel (VIO_SOLVE_MODE=0), max_iterations = 1: one full step (radius 1e4: the Gauss-Newton branch), accepted, and
    handed back through double2vector.  The returned window and landmark depths against the definition's candidate after the same gauge fix
    (solve_ref.gauge_fix), within (c)'s bound of the step carried to the outputs: with bx = s bar_z / D the bound of the tangent step,
    a position is off by at most the position bounds of its frame and of frame 0 plus |p_i - p_0| times the rotation bound of frame 0 (the
    yaw of the gauge fix), a rotation matrix entry by the rotation bounds of its frame and of frame 0, a velocity likewise, a bias by its own
    bound, a depth 1 / lambda by bl / lambda^2; a factor 2 covers the 1-norm against 2-norm slack and the yaw's dependence on pitch and roll
    (below 3 degrees here), 64 eps the conversions.  And the definition's cost at the returned window is at most that at x0."""
    cfg = cfg_of(P, name)
    pb = R.get_problem(name, cfg)
    b = handle(P, monkeypatch, name, "fallback", max_iterations=1)
    assert b.solver_kind() == 0
    stage(P, b, name)
    b.solve_stage_run(-1)
    assert b.status(0).code >= 0
    w, lm = b.window(0), b.landmarks(0)
    X0, feat0 = pb.x0()
    lin, st = R.lin_at(name, cfg, X0, feat0)
    bar, ref = R.bars(pb, X0, feat0, st, R.RADIUS0)
    assert ref["branch"] == "gn"
    Xc, cf, _, _, _ = R.candidate(pb, X0, feat0, st.s, ref["y"])
    fc, efc = R.cost(pb, Xc, cf)
    assert R.step_control(lin.cost, fc, ref["model_change"], R.RADIUS0, float(ref["norm"]))[0]
    Pn, Rn, Vn = R.gauge_fix(X0, Xc)
    na, W1 = len(pb.act), pb.W1
    bz = np.broadcast_to(bar["z"], (st.N,))
    bxa = D._f64(st.s) * bz / D._f64(st.Dg)
    bx = np.zeros(pb.P)
    bx[pb.act] = bxa[:na]
    eth0 = bx[3:6].sum()
    q = {}
    for i in range(W1):
        bp, bt, bv = bx[6 * i:6 * i + 3].sum(), bx[6 * i + 3:6 * i + 6].sum(), bx[pb.oS + 9 * i:pb.oS + 9 * i + 3].sum()
        dp = float(np.linalg.norm(D._f64(Pn[i] - Pn[0])))
        tp = 2 * (bp + bx[:3].sum()) + 2 * dp * eth0 + 64 * EPS * (1 + np.abs(w[i, :3]).max())
        tr = 2 * (bt + eth0) + 64 * EPS
        tv = 2 * bv + 2 * float(np.linalg.norm(D._f64(Vn[i]))) * eth0 + 64 * EPS * (1 + np.abs(w[i, 7:10]).max())
        q["P"] = max(q.get("P", 0), R.ratio(w[i, :3], Pn[i], tp))
        q["R"] = max(q.get("R", 0), R.ratio(_rotm(w[i, 3:7]), Rn[i], tr))
        q["V"] = max(q.get("V", 0), R.ratio(w[i, 7:10], Vn[i], tv))
        q["bias"] = max(q.get("bias", 0), R.ratio(w[i, 10:16], Xc["sb"][i, 3:], bx[pb.oS + 9 * i + 3:pb.oS + 9 * i + 9] + 4 * EPS * np.abs(Xc["sb"][i, 3:])))
    order = [int(x) for x in R.get_case(name, cfg)["st"]["lm_order"]]
    row = {slot: k for k, slot in enumerate(order)}
    depth = np.array([lm[row[slot], 3] for slot in pb.plist])
    bl = np.zeros(pb.F)
    bl[pb.var] = bxa[na:]
    q["depth"] = R.ratio(depth, 1 / cf.astype(L), 2 * bl / cf ** 2 + 8 * EPS / np.abs(cf))
    note(q, name, "fallback/f")
    # the definition's cost at the returned window
    Xr = dict(pose=np.hstack([w[:, :3], w[:, 4:7], w[:, 3:4]]), sb=w[:, 7:16].copy(), ex=X0["ex"], td=X0["td"])
    fr_, er = R.cost(pb, Xr, 1.0 / depth)
    assert float(fr_) - er <= float(lin.cost) + lin.cost_bound, (float(fr_), float(lin.cost))


def _bits(o):
    keys = ("H", "g", "sp", "Hpl", "Hll", "gl", "sl", "gnp", "gnl", "stp", "stl", "dgp", "dgl", "feat", "cfeat", "var_slots")
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in keys) + b"".join(
        np.ascontiguousarray(o[x][k]).tobytes() for x in ("X", "Xc") for k in ("pose", "sb", "ex")) + repr(
        [o[k] for k in ("stage", "iter", "F", "Fa", "nres", "cost", "radius", "mu", "alpha", "dogleg_norm", "model_change")]).encode()


@pytest.mark.parametrize("kind", ["default", "fuse"])
def test_two_staged_sequences_beside_an_idle_one(P, monkeypatch, kind):
    """sequences 0 and 2 staged with Fa = 3 and Fa = 17, sequence 1 idle; with a radius written by the harness (which writes it to staged sequences only)"""
    na, nb = "Fa3_W4", "Fa17_W4"
    single = []
    for nm in (na, nb):
        b = handle(P, monkeypatch, nm, kind)
        stage(P, b, nm)
        b.solve_stage_run(0, "serial", radius0=300.0)
        single.append(b.solve_stage_get(0))
    b3 = handle(P, monkeypatch, na, kind, S=3)
    b3.reset_seq(1)
    idle0 = b3.save([1])[0].copy()
    stage(P, b3, na, 0)
    stage(P, b3, nb, 2)
    b3.solve_stage_run(0, "serial", radius0=300.0)
    o0, o2, o1 = b3.solve_stage_get(0), b3.solve_stage_get(2), b3.solve_stage_get(1)
    assert _bits(o0) == _bits(single[0]) and _bits(o2) == _bits(single[1])
    assert o1["stage"] == "idle"
    idle1 = b3.save([1])[0]
    assert idle0.size == idle1.size and np.array_equal(idle0, idle1), int(np.count_nonzero(idle0 != idle1))


def _broken(st, what, W, NL):
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    live = [int(x) for x in s["lm_order"]]
    if what == "est_flag_3":
        s["lm_est_flag"][live[0]] = 3
    elif what == "est_flag_negative":
        s["lm_est_flag"][live[1]] = -1
    elif what == "slot_ge_NL":
        s["lm_order"][0] = NL
    elif what == "slot_twice":
        s["lm_order"][2] = s["lm_order"][0]
    elif what == "n_lm_gt_NL":
        s["n_lm"] = NL + 1
    elif what == "nobs_past_window":
        s["lm_nobs"][live[0]] = W + 2 - s["lm_start"][live[0]]
    elif what == "start_negative":
        s["lm_start"][live[1]] = -1
    elif what == "samples_65":
        s["imu_n"][2] = 65
    elif what == "headers_equal":
        s["Headers"][2] = s["Headers"][1]
    elif what == "depth_nan":
        s["lm_depth"][live[0]] = np.nan
    elif what == "pre_idx_twice":
        s["pre_idx"][0] = s["pre_idx"][1]
    elif what == "ring_base_range":
        s["ring_base"] = W + 1
    elif what == "prior_nan":
        s["prior"] = dict(s["prior"], H=s["prior"]["H"].copy())
        s["prior"]["H"][3, 3] = np.nan
    else:
        raise ValueError(what)
    return s


MALFORMED = ["est_flag_3", "est_flag_negative", "slot_ge_NL", "slot_twice", "n_lm_gt_NL", "nobs_past_window", "start_negative", "samples_65",
             "headers_equal", "depth_nan", "pre_idx_twice", "ring_base_range", "prior_nan"]


def test_malformed_tables_are_refused_and_nothing_runs(P, monkeypatch):
    """every kind of inconsistency is VIO_EINVAL before anything is written: the sequence's blob is unchanged and a run afterwards finds nothing to
    solve.  More residuals than the residual list holds, or landmarks than NL, cannot be reached through the ABI with tables of NL slots and
    windows of at most 20 frames on the handles of this file (NRES >= W NP + 2 NL); the residual count against the evaluation launch can:"""
    name = "base_W4"
    cfg = cfg_of(P, name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    b = P.VioBatch(cfg, 1)
    try:
        NL = b.capacity()["landmarks"]
        st = D.pad_tables(R.get_case(name, cfg)["st"], NL)
        before = b.save([0])[0].copy()
        for what in MALFORMED:
            with pytest.raises(P.VioError) as e:
                b.solve_stage_set(0, _broken(st, what, 4, NL))
            assert "(-1)" in str(e.value), (what, str(e.value))
            assert np.array_equal(before, b.save([0])[0]), what
        b.solve_stage_run(0, "serial")
        assert b.solve_stage_get(0)["stage"] == "idle" and np.array_equal(before, b.save([0])[0])
        for bad in (dict(slots=0, stop="schur", radius0=-1.0), dict(slots=int(cfg.max_iterations) + 2, stop="asm_a"), dict(slots=-1, stop="schur")):
            with pytest.raises(P.VioError):
                b.solve_stage_run(**bad)
        # and the same handle takes the well-formed state afterwards
        b.solve_stage_set(0, st)
        b.solve_stage_run(0, "schur")
        assert b.solve_stage_get(0)["stage"] == "asm"
    finally:
        b.close()
    # more residuals than the handle covers: every slot a full track on a handle sized for 30 features per frame
    b = P.VioBatch(P.canonical_config(**dict(R.cfg_kwargs(name), max_cnt=30)), 1)
    try:
        NL = b.capacity()["landmarks"]
        big = D.pad_tables(R.get_case(name, cfg)["st"], NL)
        big = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in big.items()}
        big["lm_order"] = np.arange(NL, dtype=np.int32)
        big["lm_start"][:], big["lm_nobs"][:], big["lm_dyn"][:], big["lm_depth"][:] = 0, 5, 0, 3.0
        before = b.save([0])[0].copy()
        with pytest.raises(P.VioError) as e:
            b.solve_stage_set(0, big)
        assert "residuals" in str(e.value) and np.array_equal(before, b.save([0])[0])
    finally:
        b.close()


def test_zz_report_worst_ratios():
    print("WORST device error / bound:", " ".join("%s=%.3g" % kv for kv in sorted(_worst.items())))
