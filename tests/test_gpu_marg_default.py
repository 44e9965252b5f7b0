"""The default marginalisation (marg_exact = 0) as the shipped kernels run it -- be_marg_kernel (reduced system in LDS), be_marg_hbm_kernel and the
be_marg_pre_kernel + be_marg_alg_kernel pair, with 256 and 512 threads -- against its definition (tests/marg_default_ref.py: factors from
factor_ref, reduction in extended precision, bounds derived there) on staged window states: vio_debug_marg_set writes a generated state into a real
handle, vio_debug_marg_run launches what vio_feed launches behind the solve, vio_debug_marg_get reads the result.  One launch per run.

Per case and handle: (a) on HBM handles the reduced system over q (margA / margB), A_r (margV) and b_r against the reference within their bounds;
(b) prior_H, prior_r, prior_c0 within theirs, prior_H exactly symmetric; (c) prior_x0 equal to the staged parameters -- bit for bit where a
parameter is staged as such (positions, speed-bias, extrinsic translation, td), within 8 eps where it passes through the device's matrix ->
quaternion conversion (the window is staged as rotation matrices; the reference converts in long double); (d) prior_present and has_prior equal to
the definition's; (e) LDS, HBM and split handles of one thread count return the same bits.  c0 is compared twice: with the reference's c0 where
the definition bounds it (31 of the 45 cases that marginalise; the 14 others by name in tests/test_marg_default_ref_cpu.py), and in every case with c0 formed in mpmath from
the prior_H and prior_r the kernel RETURNED (marg_default_ref.c0_self: the lift and the Cholesky solve held to their own forward error) -- except
the six first marginalisations without a prior (marg_default_ref.C0_UNDETERMINED, reason there), where only c0 >= 0 and finite is asserted.
Then: (f) two sequences staged at different F0 beside an idle one equal their single-sequence runs bit for bit, (g) the idle one's snapshot blob is unchanged, (h) a malformed table is
refused and nothing runs.

Worst device error / bound over all cases and handles, measured on an MI355X (test_zz_report_worst_ratios prints them; per kind of case in
DESIGN.md section 5a): reduced system A 0.026, b 0.017; A_r 0.026, b_r 0.0077; prior_H 0.025, prior_r 0.0077, prior_c0 0.00055 against the reference and
0.0011 against c0_self.  The whole file takes about twenty-five seconds, the references (shared by every test of the session) included."""
import numpy as np
import pytest

import marg_default_ref as D

pytestmark = pytest.mark.gpu

KNOBS = ("VIO_MARG_SPLIT", "VIO_MARG_LDS", "VIO_MARG_THREADS", "VIO_GROUP_SEQS", "VIO_SOLVE_MODE")
_handles = {}
_worst = {}
EPS = D.EPS


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for b in _handles.values():
        b.close()
    _handles.clear()


def handle(P, monkeypatch, name, kind, nt, S=1):
    """a handle of the case's configuration that launches `kind` (lds | hbm | split) with nt marginalisation threads; cached for the module"""
    ck = D.cfg_kwargs(name)
    key = (tuple(sorted(ck.items())), kind, nt, S)
    if key not in _handles:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("VIO_MARG_LDS", "0" if kind == "hbm" else "1")
        monkeypatch.setenv("VIO_MARG_SPLIT", "1" if kind == "split" else "0")
        monkeypatch.setenv("VIO_MARG_THREADS", str(nt))
        b = P.VioBatch(P.canonical_config(**ck), S)
        if kind == "split":
            b.set_tracker_lag(1)
        _handles[key] = b
    return _handles[key]


def kinds_of(name):
    W = D.CASES[name][0]
    if W > 10:
        return ["hbm"]                                   # the reduced system of these windows does not fit LDS
    if not D.cfg_kwargs(name)["use_imu"]:
        return ["lds", "hbm"]                            # handles without an IMU keep the one launch
    return ["lds", "hbm", "split"]


def run_case(P, monkeypatch, name, kind, nt, b=None, seq=0, run=True, staged=1):
    cfg = P.canonical_config(**D.cfg_kwargs(name))
    b = b or handle(P, monkeypatch, name, kind, nt)
    st = D.pad_tables(D.get_case(name, cfg)["st"], b.capacity()["landmarks"])
    split0 = b.marg_split_stats() if kind == "split" else 0
    b.marg_stage_set(seq, st)
    if not run:
        return None
    b.marg_stage_run()
    o = b.marg_stage_get(seq)
    assert o["hbm"] == (kind == "hbm")
    ref = D.get_ref(name, cfg)
    if kind == "split":
        assert b.marg_split_stats() - split0 == (0 if ref.noop else staged), "the split pair did not run"
    assert b.status(seq).code >= 0
    return o


def check(name, ref, st, o, tag):
    W, n = ref.W, ref.n
    if ref.noop:
        # MARGIN_SECOND_NEW without pose W-1 in the prior: nothing is touched
        pr = st["prior"]
        assert o["has_prior"] == ref.has_prior and np.array_equal(o["prior_present"], ref.present)
        assert (o["dbg"] == -1).all()
        want = (pr["H"], pr["r"], pr["x0"]) if pr is not None else (np.zeros((n, n)), np.zeros(n), np.zeros(7 * W + 17))
        for got, w in zip((o["prior_H"], o["prior_r"], o["prior_x0"]), want):
            assert np.array_equal(got, w)
        return
    assert o["dbg"][0] == 0 and o["dbg"][2] == int(ref.second_new)
    assert np.isfinite(o["prior_H"]).all() and np.isfinite(o["prior_r"]).all() and np.isfinite(o["prior_c0"])
    assert np.array_equal(o["prior_H"], o["prior_H"].T)                                         # (b)
    kw = {}
    if o["hbm"]:
        kw = dict(A=o["margA"], b=o["margB"], Ar=o["margV"], br=o["b_r"])                        # (a)
    q = D.ratios(ref, o["prior_H"], o["prior_r"], o["prior_c0"], **kw)
    cs = D.c0_self_ratio(name, o["prior_H"], o["prior_r"], o["prior_c0"])      # asserts that the bound exists outside C0_UNDETERMINED
    if cs is not None:
        q["c0_self"] = cs
    print("MEASURED device", name, tag, " ".join("%s=%.3g" % kv for kv in sorted(q.items())))
    for k, v in q.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    assert max(q.values()) <= 1.0, (name, tag, q)
    assert o["prior_c0"] >= 0.0
    x0 = o["prior_x0"]                                                                         # (c)
    assert np.array_equal(x0[~ref.x0_quat], ref.x0[~ref.x0_quat]), np.flatnonzero(x0 != ref.x0)
    assert np.abs(x0[ref.x0_quat] - ref.x0[ref.x0_quat]).max() <= 8 * EPS
    assert np.array_equal(o["prior_present"], ref.present), (o["prior_present"], ref.present)   # (d)
    assert o["has_prior"] == 1


def same_bits(a, b):
    for k in ("prior_H", "prior_r", "prior_x0", "prior_present", "dbg"):
        if k == "dbg":
            if not np.array_equal(a[k][[0, 2]], b[k][[0, 2]]):      # (dbg[1], dbg[3] are tick counts, dbg[4] belongs to the literal modes)
                return k
        elif a[k].tobytes() != b[k].tobytes():
            return k
    if np.float64(a["prior_c0"]).tobytes() != np.float64(b["prior_c0"]).tobytes() or a["has_prior"] != b["has_prior"]:
        return "c0"
    return None


@pytest.mark.parametrize("nt", [256, 512])
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_against_the_definition(P, monkeypatch, name, nt):
    cfg = P.canonical_config(**D.cfg_kwargs(name))
    ref, st = D.get_ref(name, cfg), D.get_case(name, cfg)["st"]
    outs = {}
    for kind in kinds_of(name):
        outs[kind] = run_case(P, monkeypatch, name, kind, nt)
        check(name, ref, st, outs[kind], "%s/%d" % (kind, nt))
    first = next(iter(outs))
    for kind, o in outs.items():                                                               # (e)
        assert same_bits(outs[first], o) is None, (name, first, kind, same_bits(outs[first], o))


@pytest.mark.parametrize("kind", ["lds", "hbm", "split"])
def test_two_staged_sequences_beside_an_idle_one(P, monkeypatch, kind):
    """(f), (g): sequences 0 and 2 staged at F0 = 5 and F0 = 17, sequence 1 idle"""
    na, nb, nt = "F0_5_W4", "F0_17_W4", 512
    single = [run_case(P, monkeypatch, nm, kind, nt) for nm in (na, nb)]
    b3 = handle(P, monkeypatch, na, kind, nt, S=3)
    b3.reset_seq(1)
    idle0 = b3.save([1])[0].copy()
    run_case(P, monkeypatch, na, kind, nt, b=b3, seq=0, run=False)
    o2 = run_case(P, monkeypatch, nb, kind, nt, b=b3, seq=2, staged=2)
    o0 = b3.marg_stage_get(0)
    assert same_bits(single[0], o0) is None and same_bits(single[1], o2) is None, (same_bits(single[0], o0), same_bits(single[1], o2))
    if kind == "hbm":
        for k in ("margA", "margB", "margV", "b_r"):
            assert single[0][k].tobytes() == o0[k].tobytes() and single[1][k].tobytes() == o2[k].tobytes(), k
    idle1 = b3.save([1])[0]
    assert idle0.size == idle1.size and np.array_equal(idle0, idle1), int(np.count_nonzero(idle0 != idle1))
    assert b3.marg_stage_get(1)["has_prior"] == 0


def _broken(st, what, W, NL):
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    live = [int(x) for x in s["lm_order"]]
    if what == "slot_ge_NL":
        s["lm_order"][0] = NL
    elif what == "slot_negative":
        s["lm_order"][1] = -1
    elif what == "slot_twice":
        s["lm_order"][2] = s["lm_order"][0]
    elif what == "n_lm_gt_NL":
        s["n_lm"] = NL + 1
    elif what == "nobs_zero":
        s["lm_nobs"][live[0]] = 0
    elif what == "nobs_past_window":
        s["lm_nobs"][live[0]] = W + 2 - s["lm_start"][live[0]]
    elif what == "start_negative":
        s["lm_start"][live[1]] = -1
    elif what == "start_past_window":
        s["lm_start"][live[1]] = W + 1
    elif what == "samples_65":
        s["imu_n"][2] = 65
    elif what == "samples_negative":
        s["imu_n"][1] = -1
    elif what == "headers_equal":
        s["Headers"][2] = s["Headers"][1]
    elif what == "headers_decreasing":
        s["Headers"][W] = s["Headers"][0] - 1.0
    elif what == "depth_nan":
        s["lm_depth"][live[0]] = np.nan
    elif what == "depth_inf":
        s["lm_depth"][live[2]] = np.inf
    elif what == "pre_idx_twice":
        s["pre_idx"][0] = s["pre_idx"][1]
    elif what == "pre_idx_range":
        s["pre_idx"][0] = W + 1
    elif what == "ring_base_range":
        s["ring_base"] = W + 1
    elif what == "prior_nan":
        s["prior"] = dict(s["prior"], H=s["prior"]["H"].copy())
        s["prior"]["H"][3, 3] = np.nan
    elif what == "flag_2":
        s["marginalization_flag"] = 2
    else:
        raise ValueError(what)
    return s


MALFORMED = ["slot_ge_NL", "slot_negative", "slot_twice", "n_lm_gt_NL", "nobs_zero", "nobs_past_window", "start_negative", "start_past_window", "samples_65",
             "samples_negative", "headers_equal", "headers_decreasing", "depth_nan", "depth_inf", "pre_idx_twice", "pre_idx_range", "ring_base_range",
             "prior_nan", "flag_2"]


def test_malformed_tables_are_refused_and_nothing_runs(P, monkeypatch):
    """(h): every kind of inconsistency is VIO_EINVAL before anything is written -- the sequence's blob is unchanged, and a run afterwards leaves the
    sequence without a prior.  F0 <= NRES / W cannot be violated through the ABI (NRES >= W NP + 2 NL >= W NL): the check is there for the day the
    sizing changes."""
    name = "F0_5_W4"
    cfg = P.canonical_config(**D.cfg_kwargs(name))
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    b = P.VioBatch(cfg, 1)
    try:
        NL = b.capacity()["landmarks"]
        st = D.pad_tables(D.get_case(name, cfg)["st"], NL)
        before = b.save([0])[0].copy()
        for what in MALFORMED:
            with pytest.raises(P.VioError) as e:
                b.marg_stage_set(0, _broken(st, what, 4, NL))
            assert "(-1)" in str(e.value), (what, str(e.value))
            after = b.save([0])[0]
            assert np.array_equal(before, after), what
        b.marg_stage_run()
        o = b.marg_stage_get(0)
        assert o["has_prior"] == 0 and not o["prior_H"].any() and np.array_equal(before, b.save([0])[0])
        # and the same handle takes the well-formed state afterwards
        b.marg_stage_set(0, st)
        b.marg_stage_run()
        check(name, D.get_ref(name, cfg), st, b.marg_stage_get(0), "after-refusals")
    finally:
        b.close()


def test_literal_handles_are_refused(P, monkeypatch):
    cfg = P.canonical_config(**dict(D.cfg_kwargs("F0_5_W4"), marg_exact=2))
    b = P.VioBatch(cfg, 1)
    try:
        st = D.pad_tables(D.get_case("F0_5_W4", P.canonical_config(**D.cfg_kwargs("F0_5_W4")))["st"], b.capacity()["landmarks"])
        with pytest.raises(P.VioError):
            b.marg_stage_set(0, st)
    finally:
        b.close()


def test_zz_report_worst_ratios():
    print("WORST device error / bound:", " ".join("%s=%.3g" % kv for kv in sorted(_worst.items())))
