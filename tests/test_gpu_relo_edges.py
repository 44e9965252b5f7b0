"""vio_set_relo_frame and the solve that carries relocalisation factors on the cases of tests/relo_cases.py, frame by frame against the oracle
with the HIP path's formulations switched on (OVIO_DEVIATIONS = 31), one sequence through vio_process_obs.  tests/test_relo_cases_cpu.py shows
on the oracle alone that every case reaches the branch it is named for.

After EVERY frame the checks of test_gpu_backend_edges.compare_frame (decisions, landmark tables and window stamps equal; window and prior to
bars; overflow_flags == 0) and pending / local_index / n_factors equal.  The oracle is handed the very request the HIP handle gets (the
arguments are resolved once, on the oracle).  relo_pose right after the request, and relative_t / q / yaw, drift_t / r and relo_pose after the
solve, to bars.  Every stream goes on for at least four frames after the relocalisation solve.

BARS: ten times what the MI355X measured, rounded up to one digit, never above 1e-6 m (positions) or 1e-5 degrees (angles); DESIGN.md
section 4c repeats the table.  Then the other solver paths, a batch of three, the refusals, a reset and VO mode."""
import ctypes as C

import numpy as np
import pytest

import backend_cases as BC
import relo_cases as RC
import test_gpu_backend_edges as E
import vio_ct

pytestmark = pytest.mark.gpu

POS_CAP, ANGLE_CAP = 1e-6, 1e-5      # m, degrees: no bar below may exceed them
# per case: (|dP| (m) and |dq| of the window, |dV| |dBa| |dBg|, the prior's J^T J and J^T r relative to max|J^T J|, relocalisation positions (m):
# relo_pose right after the request and after the solve, relative_t, drift_t; relocalisation angles (degrees): relative_yaw, relative_q,
# drift_r, the rotation of relo_pose).  Each is 10 x the MI355X measurement in the comment, rounded up to one digit.
BARS = {
    "index_0":                   (3e-10, 3e-9, 4e-11, 6e-8, 3e-7),    # measured dP 2.30e-11 dq 1.13e-11 | dV 2.41e-11 dBa 2.20e-10 dBg 2.41e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 5.81e-09 m ang 2.14e-08 deg
    "index_1":                   (3e-10, 3e-9, 4e-11, 9e-8, 2e-7),    # measured dP 2.40e-11 dq 1.13e-11 | dV 2.99e-11 dBa 2.20e-10 dBg 2.88e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 8.88e-09 m ang 1.64e-08 deg (the larger of the default and the fused path)
    "index_Wm2":                 (3e-10, 3e-9, 4e-11, 7e-8, 2e-7),    # measured dP 2.30e-11 dq 1.13e-11 | dV 3.06e-11 dBa 2.20e-10 dBg 2.86e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 6.13e-09 m ang 1.71e-08 deg
    "index_Wm1":                 (3e-10, 3e-9, 4e-11, 7e-8, 2e-7),    # measured dP 2.47e-11 dq 1.13e-11 | dV 2.19e-11 dBa 2.20e-10 dBg 2.41e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 6.05e-09 m ang 1.70e-08 deg
    "no_overlap":                (4e-10, 3e-9, 4e-11, 2e-8, 4e-8),    # measured dP 3.18e-11 dq 1.47e-11 | dV 3.34e-11 dBa 2.93e-10 dBg 2.41e-13 | JtJ 3.55e-12 Jtr 3.88e-13 | relo pos 1.05e-09 m ang 3.22e-09 deg
    "empty":                     (4e-10, 3e-9, 4e-11, 2e-8, 4e-8),    # measured dP 3.18e-11 dq 1.47e-11 | dV 3.34e-11 dBa 2.93e-10 dBg 2.41e-13 | JtJ 3.55e-12 Jtr 3.88e-13 | relo pos 1.05e-09 m ang 3.22e-09 deg
    "single":                    (3e-10, 3e-9, 4e-11, 4e-7, 9e-6),    # measured dP 2.30e-11 dq 1.13e-11 | dV 2.19e-11 dBa 2.20e-10 dBg 2.41e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 3.90e-08 m ang 8.98e-07 deg (below the caps: no bar of its own needed; the oracle's two formulations differ by 3.5e-08 m there)
    "ends":                      (3e-10, 3e-9, 4e-11, 8e-8, 5e-7),    # measured dP 2.96e-11 dq 1.20e-11 | dV 3.04e-11 dBa 2.42e-10 dBg 2.15e-13 | JtJ 3.12e-12 Jtr 3.86e-13 | relo pos 7.63e-09 m ang 4.65e-08 deg
    "not_in_problem":            (4e-10, 3e-9, 4e-11, 2e-8, 4e-8),    # measured dP 3.18e-11 dq 1.47e-11 | dV 3.34e-11 dBa 2.93e-10 dBg 2.41e-13 | JtJ 3.55e-12 Jtr 3.88e-13 | relo pos 1.05e-09 m ang 3.22e-09 deg
    "after_keyframe":            (8e-11, 2e-9, 2e-11, 2e-9, 4e-8),    # measured dP 6.45e-12 dq 7.14e-12 | dV 7.04e-12 dBa 1.40e-10 dBg 2.91e-14 | JtJ 1.92e-12 Jtr 2.91e-14 | relo pos 1.69e-10 m ang 3.45e-09 deg
    "after_non_keyframe":        (8e-11, 2e-9, 2e-11, 2e-8, 5e-8),    # measured dP 6.45e-12 dq 7.14e-12 | dV 7.04e-12 dBa 1.40e-10 dBg 2.91e-14 | JtJ 1.92e-12 Jtr 2.91e-14 | relo pos 1.53e-09 m ang 4.78e-09 deg
    "after_second_non_keyframe": (8e-11, 2e-9, 2e-11, 2e-8, 5e-8),    # measured dP 6.45e-12 dq 7.14e-12 | dV 7.04e-12 dBa 1.40e-10 dBg 2.91e-14 | JtJ 1.92e-12 Jtr 2.91e-14 | relo pos 1.58e-09 m ang 4.86e-09 deg
    "superseded_a":              (3e-10, 3e-9, 4e-11, 9e-8, 2e-7),    # measured dP 2.30e-11 dq 1.13e-11 | dV 2.32e-11 dBa 2.20e-10 dBg 2.41e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 8.47e-09 m ang 1.67e-08 deg
    "superseded_b":              (4e-10, 3e-9, 4e-11, 1e-8, 2e-8),    # measured dP 3.05e-11 dq 1.27e-11 | dV 2.63e-11 dBa 2.53e-10 dBg 2.41e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 9.61e-10 m ang 1.99e-09 deg
    # during_init: measured relo pos and ang 0 exactly: the identity copy is the optimum of that solve (the rig rests at the origin through the
    # initialisation), every step is rejected and both sides hand back the pose they were given; 1e-15 stands for "equal" (the comparison is <)
    "during_init":               (4e-10, 3e-9, 4e-11, 1e-15, 1e-15),  # measured dP 3.11e-11 dq 1.46e-11 | dV 3.21e-11 dBa 2.91e-10 dBg 2.41e-13 | JtJ 3.40e-12 Jtr 3.88e-13 | relo pos 0 m ang 0 deg
    "big_yaw":                   (3e-10, 3e-9, 4e-11, 9e-8, 2e-7),    # measured dP 2.40e-11 dq 1.13e-11 | dV 2.86e-11 dBa 2.20e-10 dBg 2.77e-13 | JtJ 3.36e-12 Jtr 3.88e-13 | relo pos 8.88e-09 m ang 1.64e-08 deg
    "bound":                     (8e-11, 8e-10, 2e-11, 6e-9, 2e-7),   # measured dP 7.28e-12 dq 3.96e-12 | dV 8.56e-12 dBa 7.10e-11 dBg 1.79e-14 | JtJ 1.40e-12 Jtr 8.60e-14 | relo pos 5.10e-10 m ang 1.15e-08 deg
    "td":                        (2e-11, 3e-10, 3e-12, 3e-8, 5e-9),   # measured dP 1.83e-12 dq 1.32e-12 | dV 1.58e-12 dBa 2.57e-11 dBg 4.28e-15 | JtJ 2.27e-13 Jtr 7.29e-14 | relo pos 2.24e-09 m ang 4.38e-10 deg
    "w11":                       (3e-11, 3e-10, 2e-12, 3e-9, 6e-8),   # measured dP 2.45e-12 dq 1.18e-12 | dV 1.66e-12 dBa 2.32e-11 dBg 7.20e-15 | JtJ 1.34e-13 Jtr 5.88e-14 | relo pos 2.34e-10 m ang 5.81e-09 deg
    "w20":                       (3e-11, 4e-10, 2e-12, 2e-9, 2e-7),   # measured dP 2.35e-12 dq 1.70e-12 | dV 1.95e-12 dBa 3.17e-11 dBg 4.21e-15 | JtJ 1.33e-13 Jtr 6.42e-14 | relo pos 1.15e-10 m ang 1.82e-08 deg (after the W = 20 fixes; before: dP 5.8e-04, prior JtJ 1.1)
}
OVF_RELO_DROPPED = 64                # vio_status.overflow_flags (include/vio_abi.h)
_ref, _hip = {}, {}


# ------------------------------------------------------------------------------------------------------------- pipelines
def set_relo(P, b, seq, stamp, index, mp, p, R):
    """vio_set_relo_frame through the C ABI itself (mp None: n = 0 with a NULL pointer); returns the call's code"""
    t, R = np.ascontiguousarray(p, np.float64).reshape(3), np.ascontiguousarray(R, np.float64).reshape(9)
    mp = None if mp is None else np.ascontiguousarray(mp, np.float64).reshape(-1, 3)
    return b.L.vio_set_relo_frame(b.h, seq, float(stamp), int(index), 0 if mp is None else len(mp), None if mp is None else mp.ctypes.data, t.ctypes.data,
                                  R.ctypes.data)


def hip_accessors(P):
    def record(b):
        r = E._record(b, 0)
        r["bounds"] = b.bound_stats(0)
        return r

    def set_(b, *args):
        assert set_relo(P, b, 0, *args) == P.VIO_OK, b.L.vio_last_error().decode()
    return dict(make=lambda cfg: P.VioBatch(cfg, 1), push_imu=lambda b, t, a, g: b.push_imu(0, t, a, g),
                process=lambda b, ids, obs, depth, stamp: b.process_obs(0, ids, obs, depth, stamp), record=record, relo=lambda b: b.relo(0), set_relo=set_,
                close=lambda b: b.close())


def matched_oracle(P, monkeypatch, name):
    """the matched-formulation oracle over the case, once per session; the mask is set and cleared as test_gpu_backend_edges.matched_oracle does"""
    if name not in _ref:
        case = RC.build(name, P)
        monkeypatch.setenv("OVIO_DEVIATIONS", "31")
        try:
            _ref[name] = RC.run_oracle(case, matched=True)
        finally:
            monkeypatch.delenv("OVIO_DEVIATIONS")
            vio_ct.oracle().ovio_set_deviations(0)
    return _ref[name]


def run_hip(P, case, resolved, **kw):
    return RC.drive(case, hip_accessors(P), resolved=resolved, **kw)


def hip_solo(P, monkeypatch, name):
    """the HIP run of the case on the default solver path, given the requests the oracle resolved"""
    if name not in _hip:
        ref = matched_oracle(P, monkeypatch, name)
        _hip[name] = run_hip(P, RC.build(name, P), [q["args"] for q in ref["requests"]])
    return _hip[name]


def clear_knobs(monkeypatch, **env):
    for k in E.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------------------- comparison
def _quat_deg(a, b):
    """angle between two unit quaternions given in the same component order, up to sign, from the chord (exact near zero)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.degrees(2.0 * min(np.linalg.norm(a - b), np.linalg.norm(a + b))))


def _yaw_deg(Ra, Rb):
    D = np.asarray(Ra).T @ np.asarray(Rb)
    return float(abs(np.degrees(np.arctan2(D[1, 0], D[0, 0]))))


def relo_figures(ro, rh, outputs):
    """(problems, position figure, angle figure) of two relo() results.  outputs: a relocalisation solve has written relative_* and drift_*
    (until the first one they hold what the state was created with: zeros in the HIP state, identities in the oracle); likewise relo_pose
    is compared once a request has latched"""
    bad = ["%s oracle %d hip %d" % (k, ro[k], rh[k]) for k in ("pending", "local_index", "n_factors") if ro[k] != rh[k]]
    pos, ang = 0.0, 0.0
    if outputs or ro["pending"]:
        pos = float(np.abs(ro["relo_pose"][:3] - rh["relo_pose"][:3]).max())
        ang = _quat_deg(ro["relo_pose"][3:7], rh["relo_pose"][3:7])
    if outputs:
        pos = max([pos] + [float(np.abs(ro[k] - rh[k]).max()) for k in ("relative_t", "drift_t")])
        ang = max(ang, abs((ro["relative_yaw"] - rh["relative_yaw"] + 180.0) % 360.0 - 180.0), _quat_deg(ro["relative_q"], rh["relative_q"]),
                  _yaw_deg(ro["drift_r"], rh["drift_r"]), float(np.degrees(np.abs(ro["drift_r"] - rh["drift_r"]).max())))
    return bad, pos, float(ang)


def compare_case(name, case, ref, hip, first=0):
    """worst figures over frames [first, end) and every inequality found"""
    bad, worst = E.compare_run("relo/" + name, ref["frames"][first:], hip["frames"][first:])
    worst["relo_pos"], worst["relo_ang"] = 0.0, 0.0
    sf = RC.solve_frame(case)
    pairs = [("frame %d" % k, a["relo"], b["relo"], k >= sf) for k, (a, b) in enumerate(zip(ref["frames"], hip["frames"])) if k >= first]
    pairs += [("request after frame %d" % a["after"], a["relo"], b["relo"], False) for a, b in zip(ref["requests"], hip["requests"]) if a["after"] >= first]
    for where, ro, rh, outputs in pairs:
        b, pos, ang = relo_figures(ro, rh, outputs)
        bad += ["%s: %s" % (where, x) for x in b]
        worst["relo_pos"], worst["relo_ang"] = max(worst["relo_pos"], pos), max(worst["relo_ang"], ang)
    assert len(ref["frames"]) == len(hip["frames"]) and len(ref["requests"]) == len(hip["requests"]) == len(case.requests)
    sf = RC.solve_frame(case)
    assert len(hip["frames"]) - sf > 4
    # consumed by exactly one solve
    assert hip["frames"][sf]["relo"]["pending"] == 0 and all(r["relo"]["n_factors"] == 0 and r["relo"]["pending"] == 0 for r in hip["frames"][sf + 1:])
    return bad, worst


def check_bars(name, worst, bars=None):
    print("%s: max |dP| %.2e |dq| %.2e |dV| %.2e |dBa| %.2e |dBg| %.2e  prior JtJ %.2e Jtr %.2e (own scale %.2e)  relo pos %.2e m ang %.2e deg" %
          (name, worst["P"], worst["q"], worst["V"], worst["Ba"], worst["Bg"], worst["JtJ"], worst["Jtr"], worst["Jtr_own"], worst["relo_pos"], worst["relo_ang"]))
    pose, vel, pri, rpos, rang = BARS[name] if bars is None else bars
    assert pose <= POS_CAP and pri <= 1e-5
    assert worst["P"] < pose and worst["q"] < pose, (worst["P"], worst["q"], pose)
    assert max(worst["V"], worst["Ba"], worst["Bg"]) < vel, (worst["V"], worst["Ba"], worst["Bg"], vel)
    assert worst["JtJ"] < pri and worst["Jtr"] < pri, (worst["JtJ"], worst["Jtr"], pri)
    assert worst["Jtr_own"] < E.JTR_OWN_BAR, worst["Jtr_own"]
    return rpos, rang


def check_relo_bars(name, worst, rpos, rang):
    assert rpos <= POS_CAP and rang <= ANGLE_CAP, (name, rpos, rang)
    assert worst["relo_pos"] < rpos, (worst["relo_pos"], rpos)
    assert worst["relo_ang"] < rang, (worst["relo_ang"], rang)


@pytest.mark.parametrize("name", RC.PARITY_CASES)
def test_relocalisation_case_equals_the_matched_oracle_on_every_frame(P, monkeypatch, name):
    case = RC.build(name, P)
    ref = matched_oracle(P, monkeypatch, name)
    hip = hip_solo(P, monkeypatch, name)
    bad, worst = compare_case(name, case, ref, hip)
    assert not bad, bad[:8]
    rpos, rang = check_bars(name, worst)
    check_relo_bars(name, worst, rpos, rang)
    if name in ("w11", "w20"):
        b = P.VioBatch(case.cfg, 1)
        assert b.solver_kind() == 2                                      # the streaming solver
        b.close()
    if name == "bound":
        # every clamp, bounded landmark, line-search trial and contraction counted equal, frame by frame
        for k, (ro, rh) in enumerate(zip(ref["frames"], hip["frames"])):
            assert tuple(rh["bounds"]) == tuple(ro["bounds"]) + tuple(ro["line_search"]), (k, rh["bounds"], ro["bounds"], ro["line_search"])
        sf = RC.solve_frame(case)
        assert hip["frames"][sf]["bounds"][2] > hip["frames"][sf - 1]["bounds"][2] and hip["frames"][sf]["bounds"][1] > hip["frames"][sf - 1]["bounds"][1]


# ------------------------------------------------------------------------------------------------------------- solver paths
def _masked(recs, *keys):
    """records with the named status fields removed: what a dropped request leaves different from a handle that never got one"""
    return [dict(r, status={k: v for k, v in r["status"].items() if k not in keys}) for r in recs]


def _assert_relo_identical(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        for key, v in ra["relo"].items():
            assert np.array_equal(np.asarray(v), np.asarray(rb["relo"][key])), (k, key)


def test_index_1_on_a_fused_handle_switches_to_both_launch_paths(P, monkeypatch):
    """VIO_FUSE = 1: until the request the handle launches the fused kernel alone (compact records, no room for a relocalisation factor);
    vio_set_relo_frame arms the two-kernel path beside it (relo_frames).  Before the request: a fused handle that never gets one, bit for bit.
    From the relocalisation frame on: index_1's bars against the oracle"""
    case = RC.build("index_1", P)
    ref = matched_oracle(P, monkeypatch, "index_1")
    clear_knobs(monkeypatch, VIO_FUSE="1")
    probe = P.VioBatch(case.cfg, 1)
    assert probe.solver_kind() == 1
    probe.close()
    k = case.requests[0].after
    hip = run_hip(P, case, [q["args"] for q in ref["requests"]])
    twin = run_hip(P, case, None, frames=k + 1, skip_requests=True)
    E._assert_bit_identical(hip["frames"][:k + 1], twin["frames"])
    _assert_relo_identical(hip["frames"][:k + 1], twin["frames"])
    bad, worst = compare_case("index_1", case, ref, hip)
    assert not bad, bad[:8]
    rpos, rang = check_bars("index_1", worst)
    check_relo_bars("index_1", worst, rpos, rang)
    assert hip["frames"][k + 1]["relo"]["n_factors"] == ref["frames"][k + 1]["relo"]["n_factors"] > 0


def _dropped_request_equals_a_twin(P, case, resolved):
    """the request is dropped by the next processed frame: overflow bit 64 on exactly that frame, pending == 0 and no factors after it, and
    every record equal, bit for bit, to a handle that never got the request"""
    hip = run_hip(P, case, resolved)
    twin = run_hip(P, case, None, skip_requests=True)
    k = case.requests[0].after
    assert hip["requests"][0]["relo"]["pending"] == 1
    flags = [r["status"]["overflow_flags"] for r in hip["frames"]]
    assert flags == [0] * (k + 1) + [OVF_RELO_DROPPED] + [0] * (len(flags) - k - 2), flags
    assert hip["frames"][k + 1]["status"]["code"] == P.VIO_ECAPACITY and all(r["status"]["code"] == P.VIO_OK for r in hip["frames"][k + 2:])
    assert all(r["relo"]["pending"] == 0 and r["relo"]["n_factors"] == 0 for r in hip["frames"][k + 1:])
    assert all(r["status"]["overflow_flags"] == 0 for r in twin["frames"])
    E._assert_bit_identical(_masked(hip["frames"], "overflow_flags", "overflow_frames", "code"), _masked(twin["frames"], "overflow_flags", "overflow_frames", "code"))
    assert hip["frames"][-1]["status"]["overflow_frames"] == 1 and hip["frames"][-1]["status"]["solver_flag"] == 1
    return hip


def test_index_1_on_the_persistent_solver_drops_the_request(P, monkeypatch):
    case = RC.build("index_1", P)
    ref = matched_oracle(P, monkeypatch, "index_1")
    clear_knobs(monkeypatch, VIO_SOLVE_MODE="0")
    probe = P.VioBatch(case.cfg, 1)
    assert probe.solver_kind() == 0
    probe.close()
    _dropped_request_equals_a_twin(P, case, [q["args"] for q in ref["requests"]])


def test_vo_mode_drops_the_request(P, monkeypatch):
    """use_imu = 0: solve_epilogue's VO branch hands nothing back but the poses, so a request carried into a VO solve would never be consumed
    and relo_Pose would never move.  The declared limit (include/vio_abi.h) is enforced in solve_prologue: dropped, bit 64"""
    case = RC.build("vo", P)
    clear_knobs(monkeypatch)
    o = RC.run_oracle(case)                                             # (only to resolve the request: the oracle is the literal reference here)
    hip = _dropped_request_equals_a_twin(P, case, [q["args"] for q in o["requests"]])
    assert hip["requests"][0]["relo"]["local_index"] == 1 and all(np.all(np.isfinite(r["window"])) for r in hip["frames"])


# ------------------------------------------------------------------------------------------------------------- batch
def _batch_of_three(P, cases, requests):
    """three cases of one configuration in one handle through process_obs_batch; requests[s] = resolved arguments for slot s or None.
    Per slot the drive() result: frames (record + relo) and requests"""
    cfg = cases[0].cfg
    b = P.VioBatch(cfg, 3)
    cap, H, Wd = BC.tracker_capacity(cfg), cfg.height, cfg.width
    fr = [c.stream.frames() for c in cases]
    out = [dict(frames=[], requests=[]) for _ in cases]
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
                out[s]["frames"].append(dict(E._record(b, s), relo=b.relo(s)))
        for s in range(3):
            for rq, args in zip(cases[s].requests, requests[s] or ()):
                if rq.after == k:
                    assert set_relo(P, b, s, *args) == P.VIO_OK
                    out[s]["requests"].append(dict(after=k, args=args, relo=b.relo(s)))
    b.close()
    return out


def _assert_slot_equals_solo(slot, solo):
    E._assert_bit_identical([{k: v for k, v in r.items() if k != "bounds"} for r in slot["frames"]],
                            [{k: v for k, v in r.items() if k != "bounds"} for r in solo["frames"]])
    _assert_relo_identical(slot["frames"], solo["frames"])
    assert len(slot["requests"]) == len(solo["requests"])
    _assert_relo_identical(slot["requests"], solo["requests"])


def _no_request(P, case):
    key = "none/" + case.name
    if key not in _hip:
        _hip[key] = run_hip(P, case, None, skip_requests=True)
    return _hip[key]


def test_a_request_to_one_slot_of_a_batch_leaves_the_others_alone(P, monkeypatch):
    """slot 1 of three gets index_1's request: slots 0 and 2 equal their solo runs without a request at every frame, bit for bit, slot 1 its solo
    run with it"""
    clear_knobs(monkeypatch)
    cases = [RC.build("single", P), RC.build("index_1", P), RC.build("ends", P)]
    solo = hip_solo(P, monkeypatch, "index_1")
    out = _batch_of_three(P, cases, [None, [q["args"] for q in solo["requests"]], None])
    _assert_slot_equals_solo(out[1], solo)
    assert out[1]["frames"][RC.solve_frame(cases[1])]["relo"]["n_factors"] > 0
    for s in (0, 2):
        _assert_slot_equals_solo(out[s], _no_request(P, cases[s]))
        assert all(r["relo"]["pending"] == 0 and r["relo"]["n_factors"] == 0 for r in out[s]["frames"])


def test_two_slots_of_a_batch_with_requests_of_different_length_on_the_same_frame(P, monkeypatch):
    """slots 0 and 2 get requests after the same frame, 1 and 69 match points: each reads its own row of relo_mp and equals its solo run"""
    clear_knobs(monkeypatch)
    cases = [RC.build("single", P), RC.build("no_overlap", P), RC.build("index_Wm2", P)]
    assert cases[0].requests[0].after == cases[2].requests[0].after
    solos = [hip_solo(P, monkeypatch, "single"), None, hip_solo(P, monkeypatch, "index_Wm2")]
    req = [[q["args"] for q in solos[0]["requests"]], None, [q["args"] for q in solos[2]["requests"]]]
    assert len(req[0][0][2]) == 1 and len(req[2][0][2]) > 60
    out = _batch_of_three(P, cases, req)
    _assert_slot_equals_solo(out[0], solos[0])
    _assert_slot_equals_solo(out[2], solos[2])
    _assert_slot_equals_solo(out[1], _no_request(P, cases[1]))
    sf = RC.solve_frame(cases[0])
    assert (out[0]["frames"][sf]["relo"]["n_factors"], out[1]["frames"][sf]["relo"]["n_factors"]) == (1, 0) and out[2]["frames"][sf]["relo"]["n_factors"] > 60


# ------------------------------------------------------------------------------------------------------------- refusals, reset
def test_refused_requests_leave_the_handle_untouched(P, monkeypatch):
    """n = NP + 1: VIO_ECAPACITY; ids that do not ascend (swapped, duplicated): VIO_EINVAL with a text; n > 0 with a NULL pointer: VIO_EINVAL.
    After each refusal nothing is pending and the next three frames equal, bit for bit, those of a twin handle that saw no such call"""
    clear_knobs(monkeypatch)
    case = RC.build("index_1", P)
    ref = matched_oracle(P, monkeypatch, "index_1")
    stamp, index, mp, p, R = ref["requests"][0]["args"]
    NP = BC.tracker_capacity(case.cfg)
    big = np.c_[np.zeros((NP + 1, 2)), np.arange(NP + 1, dtype=np.float64)]
    swapped, dup = mp.copy(), mp.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    dup[-1, 2] = dup[-2, 2]
    t, Rf = np.ascontiguousarray(p), np.ascontiguousarray(R).reshape(9)
    a, b = P.VioBatch(case.cfg, 1), P.VioBatch(case.cfg, 1)
    assert a.capacity()["tracks"] == NP
    fr = case.stream.frames()
    k0 = case.requests[0].after
    calls = {k0 - 6: [(big, P.VIO_ECAPACITY, "match points")], k0 - 3: [(swapped, P.VIO_EINVAL, "ascend"), (dup, P.VIO_EINVAL, "ascend")], k0: [(None, P.VIO_EINVAL, None)]}
    for k, (stamp_k, ids, obs, depth, (ti, ai, gi)) in enumerate(fr[:k0 + 4]):
        for h in (a, b):
            h.push_imu(0, ti, ai, gi)
            h.process_obs(0, ids, obs, depth, stamp_k)
        ra, rb = dict(E._record(a, 0), relo=a.relo(0)), dict(E._record(b, 0), relo=b.relo(0))
        E._assert_bit_identical([ra], [rb])
        _assert_relo_identical([ra], [rb])
        assert ra["relo"]["pending"] == 0 and ra["relo"]["n_factors"] == 0 and ra["status"]["overflow_flags"] == 0
        for arr, code, text in calls.get(k, ()):
            st = float(a.window(0)[1, 16])                               # a stamp that IS in the window: only the refusal keeps the request out
            n, ptr = (len(arr), arr.ctypes.data) if arr is not None else (3, None)
            assert a.L.vio_set_relo_frame(a.h, 0, st, index, n, ptr, t.ctypes.data, Rf.ctypes.data) == code
            if text is not None:
                assert text in a.L.vio_last_error().decode()
            assert a.relo(0)["pending"] == 0
    assert ra["status"]["solver_flag"] == 1 and ra["status"]["frames_processed"] == k0 + 4
    a.close()
    b.close()


def test_reset_seq_discards_a_pending_request(P, monkeypatch):
    """a latched request, then vio_reset_seq: nothing pending, and the rest of the stream comes out as on a fresh handle, bit for bit"""
    clear_knobs(monkeypatch)
    case = RC.build("index_1", P)
    ref = matched_oracle(P, monkeypatch, "index_1")
    fr, k0 = case.stream.frames(), 9
    a, b = P.VioBatch(case.cfg, 1), P.VioBatch(case.cfg, 1)
    for stamp, ids, obs, depth, (ti, ai, gi) in fr[:k0 + 1]:
        a.push_imu(0, ti, ai, gi)
        a.process_obs(0, ids, obs, depth, stamp)
    _, index, mp, p, R = ref["requests"][0]["args"]
    assert set_relo(P, a, 0, float(a.window(0)[1, 16]), index, mp, p, R) == P.VIO_OK
    assert a.relo(0)["pending"] == 1 and a.relo(0)["local_index"] == 1
    a.reset_seq(0)
    assert a.relo(0)["pending"] == 0
    keys = BC.STATUS_KEYS + ("has_prior", "overflow_flags", "code", "processed", "reboot_count")
    for k, (stamp, ids, obs, depth, (ti, ai, gi)) in enumerate(fr[k0 + 1:], k0 + 1):
        for h in (a, b):
            h.push_imu(0, ti, ai, gi)
            h.process_obs(0, ids, obs, depth, stamp)
        ra, rb = dict(E._record(a, 0), relo=a.relo(0)), dict(E._record(b, 0), relo=b.relo(0))
        # (the counters over the life of the handle -- frames, iterations, solves -- go on across an estimator restart)
        E._assert_bit_identical(*[[dict(r, status={q: r["status"][q] for q in keys})] for r in (ra, rb)])
        assert ra["relo"]["pending"] == 0 and ra["relo"]["n_factors"] == 0, k
    assert ra["status"]["solver_flag"] == 1 and ra["status"]["iterations"] >= 1
    a.close()
    b.close()
