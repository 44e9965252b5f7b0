"""The back-end chain (be_ingest -> solve -> be_marg -> be_finish) on the generated streams of tests/backend_cases.py, frame by frame against
the oracle with the HIP path's formulations switched on (OVIO_DEVIATIONS = 31), through vio_process_obs / OraclePipeline.process_obs.
tests/test_backend_cases_cpu.py shows on the oracle alone that every stream reaches the branch it is named for.

After EVERY frame: the status decisions, the integer columns and the first / last observations of the landmark table, the whole window
(P, q, V, Ba, Bg) and, where there is one, the prior as a quadratic form (J^T J, J^T r, present mask); overflow_flags == 0 throughout.
Decisions and tables must be equal.  The numeric bars are per case, ten times what the MI355X measured, rounded up to one significant
digit (the project's margin: 5e-9 for a measured 6e-10 on the rendered scene); BARS lists them with the measurements, DESIGN.md section 3
repeats the table together with what the oracle's own two formulations leave between them on the same streams.

hash_chain hands its maps over in shuffled order.  The oracle, like the reference, receives a std::map and so appends a frame's new
landmarks in ascending id; the HIP path appends them in the order of the map it is given.  For that case the tables are compared row by row
after sorting both by id; everything else is compared as for the other cases (the order of the list only reorders sums).

imu_65 and table_full run into a capacity on purpose (the oracle's lists are unbounded): equal to the oracle before the overflow frame,
exactly the one flag on it, and the sequence goes on."""
import numpy as np
import pytest

import backend_cases as BC
import vio_ct

pytestmark = pytest.mark.gpu

# per case: (bar on |dP| (m) and |dq| (unit quaternion), bar on |dV| (m/s), |dBa| (m/s^2), |dBg| (rad/s), bar on the prior's J^T J and J^T r
# relative to max|J^T J|).  Each is 10 x the MI355X measurement in the comment -- the worst over every frame and window slot of the case, the
# larger of the figures that share a bar -- rounded up to one digit.  None: the case has no keyframe, hence no prior.
BARS = {
    "standstill":          (4e-10, 7e-9, 7e-11),   # measured dP 3.96e-11 dq 3.30e-11 | dV 8.12e-11 dBa 6.45e-10 dBg 4.68e-14 | JtJ 6.18e-12 Jtr 8.80e-14
    "standstill_short":    (8e-11, 2e-9, 2e-11),   # measured dP 6.45e-12 dq 7.14e-12 | dV 7.04e-12 dBa 1.40e-10 dBg 2.91e-14 | JtJ 1.92e-12 Jtr 2.91e-14
    "imu_counts":          (6e-9, 2e-8, 3e-8),     # measured dP 5.26e-10 dq 3.81e-11 | dV 1.03e-09 dBa 3.78e-10 dBg 1.49e-12 | JtJ 2.20e-09 Jtr 2.18e-12
    "imu_65":              (3e-14, 2e-13, None),   # measured dP 2.38e-15 dq 1.66e-15 | dV 1.37e-14 dBa 1.00e-14 dBg 5.78e-16 (the 8 frames before the overflow)
    "hash_chain":          (3e-10, 2e-9, 4e-11),   # measured dP 2.29e-11 dq 8.14e-12 | dV 2.27e-11 dBa 1.50e-10 dBg 1.25e-13 | JtJ 3.55e-12 Jtr 2.03e-13
    "reappear":            (9e-10, 2e-8, 3e-10),   # measured dP 8.25e-11 dq 7.83e-11 | dV 1.34e-10 dBa 1.62e-09 dBg 5.52e-13 | JtJ 2.83e-11 Jtr 1.85e-12
    "thin":                (2e-9, 7e-9, 2e-10),    # measured dP 1.09e-10 dq 3.31e-11 | dV 1.01e-10 dBa 6.48e-10 dBg 1.98e-13 | JtJ 1.06e-11 Jtr 1.30e-12
    "depth_edges":         (2e-10, 2e-9, 3e-11),   # measured dP 1.31e-11 dq 5.63e-12 | dV 1.46e-11 dBa 1.02e-10 dBg 1.44e-14 | JtJ 2.32e-12 Jtr 1.08e-13
    "short_tracks":        (3e-10, 2e-9, 5e-11),   # measured dP 2.06e-11 dq 8.38e-12 | dV 2.23e-11 dBa 1.61e-10 dBg 2.43e-13 | JtJ 4.38e-12 Jtr 3.86e-13
    "table_full":          (9e-11, 2e-9, 2e-11),   # measured dP 8.78e-12 dq 8.38e-12 | dV 1.83e-11 dBa 1.61e-10 dBg 4.97e-14 | JtJ 1.85e-12 Jtr 8.26e-14 (the 10 frames before the overflow)
    "w10_td":              (1e-10, 9e-10, 8e-11),  # measured dP 9.53e-12 dq 4.15e-12 | dV 5.53e-12 dBa 8.11e-11 dBg 1.05e-14 | JtJ 7.25e-12 Jtr 9.84e-14
    "standstill/fused":    (4e-10, 7e-9, 7e-11),   # measured: the figures of the default path, digit for digit
    "standstill/fallback": (6e-10, 9e-9, 1e-10),   # measured dP 5.26e-11 dq 4.32e-11 | dV 1.55e-10 dBa 8.43e-10 dBg 6.20e-14 | JtJ 9.14e-12 Jtr 2.02e-13
}
# J^T r against its OWN scale, max(1, max|J^T r|), as test_prior_matches_oracle_as_a_quadratic_form normalises it: that test's bar, for every case.
# Measured 1.0e-08 .. 2.5e-07, imu_counts 2.76e-06 (its gradient is small where frames lie 5 ms apart: the same absolute difference weighs more)
JTR_OWN_BAR = 1e-5

INT_COLS, OBS_COLS = (0, 1, 2, 4, 5, 6), (7, 8, 9, 10, 11)     # landmarks_ex: id start n_obs . estimate_flag solve_flag is_dynamic | first obs x y z depth, last depth
_ref, _hip = {}, {}


def matched_oracle(P, monkeypatch, name):
    """the matched-formulation oracle over the case, run once per session; the mask is set and cleared as
    test_pipeline_equals_the_oracle_with_matched_formulations_to_round_off does"""
    if name not in _ref:
        st = BC.build(name, P)
        monkeypatch.setenv("OVIO_DEVIATIONS", "31")
        try:
            _ref[name] = BC.run_oracle(st, matched=True)
        finally:
            monkeypatch.delenv("OVIO_DEVIATIONS")
            vio_ct.oracle().ovio_set_deviations(0)
    return _ref[name]


def _record(b, s):
    st = b.status(s)
    pr = b.prior(s)
    return dict(status={k: getattr(st, k) for k, _ in st._fields_}, window=b.window(s).copy(), lm=b.landmarks_ex(s).copy(),
                prior=None if pr is None else BC.prior_quadratic(pr, False))


def run_hip(P, st, upto=None):
    """a one-sequence VioBatch over the stream through process_obs: the same record per frame as BC.run_oracle"""
    b = P.VioBatch(st.cfg, 1)
    cap = b.capacity()
    assert (cap["tracks"], cap["landmarks"]) == (BC.tracker_capacity(st.cfg), BC.landmark_capacity(st.cfg))
    out = []
    for stamp, ids, obs, depth, (ti, ai, gi) in st.frames()[:upto]:
        if len(ti):
            b.push_imu(0, ti, ai, gi)
        b.process_obs(0, ids, obs, depth, stamp)
        out.append(_record(b, 0))
    b.close()
    return out


def hip_solo(P, name):
    if name not in _hip:
        _hip[name] = run_hip(P, BC.build(name, P))
    return _hip[name]


KNOBS = ("VIO_FUSE", "VIO_EVAL_RPT", "VIO_MARG_THREADS", "VIO_SOLVE_MODE", "VIO_FLAGS", "VIO_BE_THREADS", "VIO_LINE_SEARCH")
# the sum_dt > 10 rule is written out once per solver path: the default two-kernel path (ps_eval / ps_asm_a) runs in every test above, the
# fused evaluate + assemble kernel and the persistent fallback solver are chosen when the handle is created
SOLVER_PATHS = {"fused": ({"VIO_FUSE": "1"}, 1), "fallback": ({"VIO_SOLVE_MODE": "0"}, 0)}


def compare_frame(k, ro, rh, by_id=False):
    """(problems, figures) of one frame: problems lists what must be EQUAL and is not, figures the numeric differences"""
    bad, fig = [], {}
    so, sh = ro["status"], rh["status"]
    for key in BC.STATUS_KEYS:
        if int(so[key]) != int(sh[key]):
            bad.append("frame %d: %s oracle %d hip %d" % (k, key, int(so[key]), int(sh[key])))
    if int(so["has_prior"]) != int(sh["has_prior"]) or (ro["prior"] is None) != (rh["prior"] is None):
        bad.append("frame %d: has_prior" % k)
    lo, lh = ro["lm"], rh["lm"]
    if by_id:
        lo, lh = lo[np.argsort(lo[:, 0], kind="stable")], lh[np.argsort(lh[:, 0], kind="stable")]
    if lo.shape != lh.shape or not np.array_equal(lo[:, INT_COLS], lh[:, INT_COLS]):
        bad.append("frame %d: landmark table (integer columns)" % k)
    elif not np.array_equal(lo[:, OBS_COLS], lh[:, OBS_COLS]):
        bad.append("frame %d: first / last observations" % k)
    wo, wh = ro["window"], rh["window"]
    if not np.array_equal(wo[:, 16], wh[:, 16]):
        bad.append("frame %d: window stamps" % k)
    fig["P"] = float(np.abs(wo[:, 0:3] - wh[:, 0:3]).max())
    fig["q"] = float(np.minimum(np.abs(wo[:, 3:7] - wh[:, 3:7]).max(1), np.abs(wo[:, 3:7] + wh[:, 3:7]).max(1)).max())
    fig["V"] = float(np.abs(wo[:, 7:10] - wh[:, 7:10]).max())
    fig["Ba"] = float(np.abs(wo[:, 10:13] - wh[:, 10:13]).max())
    fig["Bg"] = float(np.abs(wo[:, 13:16] - wh[:, 13:16]).max())
    if ro["prior"] is not None and rh["prior"] is not None:
        (Ho, go, po), (Hh, gh, ph) = ro["prior"], rh["prior"]
        if not np.array_equal(po, ph):
            bad.append("frame %d: prior present mask" % k)
        fig["JtJ"] = float(np.abs(Ho - Hh).max() / max(np.abs(Ho).max(), 1e-300))
        fig["Jtr"] = float(np.abs(go - gh).max() / max(np.abs(Ho).max(), 1e-300))
        fig["Jtr_own"] = float(np.abs(go - gh).max() / max(1.0, np.abs(go).max()))
    return bad, fig


def compare_run(name, oracle_recs, hip_recs, upto=None):
    """worst figures over frames [0, upto) and every inequality found"""
    bad, worst = [], dict(P=0.0, q=0.0, V=0.0, Ba=0.0, Bg=0.0, JtJ=0.0, Jtr=0.0, Jtr_own=0.0)
    n = len(oracle_recs) if upto is None else upto
    for k in range(n):
        b, f = compare_frame(k, oracle_recs[k], hip_recs[k], by_id=(name == "hash_chain"))
        bad += b
        for key, v in f.items():
            worst[key] = max(worst[key], v)
        if hip_recs[k]["status"]["overflow_flags"] != 0:
            bad.append("frame %d: overflow_flags %d" % (k, hip_recs[k]["status"]["overflow_flags"]))
        if hip_recs[k]["status"]["code"] != 0 or hip_recs[k]["status"]["processed"] != 1:
            bad.append("frame %d: code %d processed %d" % (k, hip_recs[k]["status"]["code"], hip_recs[k]["status"]["processed"]))
    return bad, worst


def check_bars(name, worst):
    print("%s: max |dP| %.2e |dq| %.2e |dV| %.2e |dBa| %.2e |dBg| %.2e  prior JtJ %.2e Jtr %.2e (own scale %.2e)" %
          (name, worst["P"], worst["q"], worst["V"], worst["Ba"], worst["Bg"], worst["JtJ"], worst["Jtr"], worst["Jtr_own"]))
    pose, vel, pri = BARS[name]
    assert pose <= 1e-5 and (pri is None or pri <= 1e-5)   # a matched comparison worse than the suite's bar against the UNMATCHED oracle is not round-off
    assert worst["P"] < pose and worst["q"] < pose, (worst["P"], worst["q"], pose)
    assert max(worst["V"], worst["Ba"], worst["Bg"]) < vel, (worst["V"], worst["Ba"], worst["Bg"], vel)
    if pri is not None:
        assert worst["JtJ"] < pri and worst["Jtr"] < pri, (worst["JtJ"], worst["Jtr"], pri)
        assert worst["Jtr_own"] < JTR_OWN_BAR, worst["Jtr_own"]


@pytest.mark.parametrize("name", BC.PARITY_CASES)
def test_back_end_equals_the_matched_oracle_on_every_frame(P, monkeypatch, name):
    ref = matched_oracle(P, monkeypatch, name)
    hip = hip_solo(P, name)
    bad, worst = compare_run(name, ref, hip)
    assert not bad, bad[:8]
    assert sum(r["prior"] is not None for r in hip) >= 10      # (the prior was compared, not absent)
    check_bars(name, worst)


@pytest.mark.parametrize("path", list(SOLVER_PATHS))
def test_standstill_on_the_other_solver_paths(P, monkeypatch, path):
    env, kind = SOLVER_PATHS[path]
    ref = matched_oracle(P, monkeypatch, "standstill")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = BC.build("standstill", P)
    probe = P.VioBatch(st.cfg, 1)
    assert probe.solver_kind() == kind
    probe.close()
    hip = run_hip(P, st)
    bad, worst = compare_run("standstill", ref, hip)
    assert not bad, bad[:8]
    check_bars("standstill/" + path, worst)


@pytest.mark.parametrize("name", ["imu_65", "table_full"])
def test_capacity_case_flags_its_frame_and_goes_on(P, monkeypatch, name):
    """Note on status.code: vio_get_status reports VIO_ECAPACITY for a frame that raised a capacity flag (include/vio_abi.h, and
    test_gpu_ex_calib asserts it for flag 128); that is the status of the FRAME.  The call itself returns VIO_OK, the frame is processed, and the
    code is VIO_OK again on every later frame: that is what is asserted here."""
    st = BC.build(name, P)
    f, bit = st.notes["overflow_frame"], st.notes["overflow_bit"]
    ref = matched_oracle(P, monkeypatch, name)
    hip = hip_solo(P, name)                                              # (process_obs raises on any call that does not return VIO_OK)
    bad, worst = compare_run(name, ref, hip, upto=f)
    assert not bad, bad[:8]
    check_bars(name, worst)
    sf = hip[f]["status"]
    assert sf["overflow_flags"] == bit and sf["processed"] == 1 and sf["solver_flag"] == 1 and sf["code"] == P.VIO_ECAPACITY, sf
    for k in range(f + 1, len(hip)):
        s = hip[k]["status"]
        assert (s["overflow_flags"], s["code"], s["processed"], s["solver_flag"], s["reboot_count"]) == (0, P.VIO_OK, 1, 1, 0), (k, s)
        assert s["iterations"] >= 1 and np.all(np.isfinite(hip[k]["window"]))
    assert hip[-1]["status"]["overflow_frames"] == 1 and hip[-1]["status"]["frames_processed"] == len(hip)
    if name == "table_full":
        cap = BC.landmark_capacity(st.cfg)
        assert hip[f - 1]["status"]["n_landmarks"] == cap == int(ref[f - 1]["status"]["n_landmarks"])     # exactly full, and equal (compared above)
        assert hip[f]["status"]["n_landmarks"] == cap and int(ref[f]["status"]["n_landmarks"]) == cap + 1
        for k in range(f, len(hip)):      # the landmarks that did fit are the oracle's entries for the same ids, in the same order
            lo, lh = ref[k]["lm"], hip[k]["lm"]
            keep = np.isin(lo[:, 0], lh[:, 0])
            assert keep.sum() == len(lh) and len(lo) - len(lh) in (0, 1), (k, len(lo), len(lh))
            assert np.array_equal(lo[keep][:, INT_COLS], lh[:, INT_COLS]) and np.array_equal(lo[keep][:, OBS_COLS], lh[:, OBS_COLS]), k
        # the landmark that did not fit had one observation and never enters a solve: the window stays the oracle's
        tail, _ = compare_run(name, [dict(r, lm=h["lm"], status=dict(r["status"], n_landmarks=h["status"]["n_landmarks"])) for r, h in zip(ref, hip)],
                              [dict(h, status=dict(h["status"], overflow_flags=0, code=0)) for h in hip])
        assert not tail, tail[:8]


def _batch_of_three(P, streams):
    """three streams of one configuration in one handle through process_obs_batch: per frame the record of every slot that still has frames"""
    cfg = streams[0].cfg
    b = P.VioBatch(cfg, 3)
    cap, H, Wd = BC.tracker_capacity(cfg), cfg.height, cfg.width
    fr = [s.frames() for s in streams]
    out = [[] for _ in streams]
    for k in range(max(len(f) for f in fr)):
        n_obs, ids, obs = np.full(3, -1, np.int32), np.zeros((3, cap), np.int32), np.zeros((3, cap, 7))
        depth, stamps = np.zeros((3, H, Wd), np.uint16), np.zeros(3)
        for s in range(3):
            if k >= len(fr[s]):
                continue
            stamp, i, o, d, (ti, ai, gi) = fr[s][k]
            if len(ti):
                b.push_imu(s, ti, ai, gi)
            n_obs[s], ids[s, :len(i)], obs[s, :len(i)], depth[s], stamps[s] = len(i), i, o, d, stamp
        b.process_obs_batch(n_obs, ids, obs, depth, stamps)
        for s in range(3):
            if k < len(fr[s]):
                out[s].append(_record(b, s))
    b.close()
    return out


def _assert_bit_identical(a, b):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra["status"] == rb["status"], (k, ra["status"], rb["status"])
        assert np.array_equal(ra["window"], rb["window"]) and np.array_equal(ra["lm"], rb["lm"]), k
        assert (ra["prior"] is None) == (rb["prior"] is None), k
        if ra["prior"] is not None:
            assert all(np.array_equal(x, y) for x, y in zip(ra["prior"], rb["prior"])), k


def test_hash_chain_is_bit_identical_inside_a_batch(P):
    """slot 1 of three, reappear and thin beside it, through vio_process_obs_batch: every frame's record equals the solo run's bit for bit"""
    others = [BC.build("reappear", P), BC.build("thin", P)]
    out = _batch_of_three(P, [others[0], BC.build("hash_chain", P), others[1]])
    _assert_bit_identical(out[1], hip_solo(P, "hash_chain"))
    _assert_bit_identical(out[0], hip_solo(P, "reappear"))


def test_w10_td_is_bit_identical_inside_a_batch(P):
    """slot 2 of three; the other slots run the hash_chain and depth_edges streams under w10_td's configuration (a batch has one)"""
    kw = dict(window_size=10, estimate_td=1, estimate_extrinsic=1)
    out = _batch_of_three(P, [BC.hash_chain(P, **kw), BC.depth_edges(P, **kw), BC.build("w10_td", P)])
    _assert_bit_identical(out[2], hip_solo(P, "w10_td"))
    assert all(r["status"]["reboot_count"] == 0 and r["status"]["processed"] == 1 for o in out[:2] for r in o)


def test_negative_id_is_refused_on_the_host_and_leaves_the_sequence_untouched(P):
    """vio_process_obs and vio_process_obs_batch with a negative id: VIO_EINVAL with a text, nothing uploaded or launched (no kernel ever sees the
    id), and the next valid frame comes out exactly as on a handle that never saw the bad calls"""
    st = BC.build("hash_chain", P)
    fr = st.frames()[:8]
    cfg = st.cfg
    a, b = P.VioBatch(cfg, 1), P.VioBatch(cfg, 1)
    for k, (stamp, ids, obs, depth, (ti, ai, gi)) in enumerate(fr):
        for h in (a, b):
            h.push_imu(0, ti, ai, gi)
        if k in (2, 6):     # before and after initialisation
            for pos, val in ((0, -1), (len(ids) - 1, -7), (3, -2 ** 31)):
                bad = ids.copy()
                bad[pos] = val
                with pytest.raises(P.VioError, match=r"\(-1\).*negative feature id"):
                    a.process_obs(0, bad, obs, depth, stamp)
                with pytest.raises(P.VioError, match=r"\(-1\).*negative feature id"):
                    a.process_obs_batch([len(bad)], bad[None], obs[None], depth[None], [stamp])
            assert a.status(0).frames_processed == k
        a.process_obs(0, ids, obs, depth, stamp)
        b.process_obs(0, ids, obs, depth, stamp)
        ra, rb = _record(a, 0), _record(b, 0)
        _assert_bit_identical([ra], [rb])
    assert ra["status"]["solver_flag"] == 1 and ra["status"]["frames_processed"] == len(fr)
