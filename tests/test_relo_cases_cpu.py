"""The relocalisation cases of tests/relo_cases.py on the oracle alone: every case latches as it should, its relocalisation solve carries
the number of factors the case is named for, is consumed by exactly one solve and leaves everything finite -- so that the GPU comparison of
tests/test_gpu_relo_edges.py cannot pass vacuously."""
import numpy as np
import pytest

import backend_cases as BC
import relo_cases as RC

_runs = {}


def _run(P, name):
    if name not in _runs:
        case = RC.build(name, P)
        _runs[name] = (case, RC.run_oracle(case))
    return _runs[name]


def _dist(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


# expected (local index after the last request, number of factors: an int, or "all" = every in-problem landmark of the solve)
EXPECT = {
    "index_0": (0, None), "index_1": (1, "all"), "index_Wm2": (2, "all"), "index_Wm1": (3, "all"), "no_overlap": (1, 0), "empty": (1, 0), "single": (1, 1),
    "ends": (1, 2), "not_in_problem": (0, 0), "after_keyframe": (1, "all"), "after_non_keyframe": (1, "all"), "after_second_non_keyframe": (1, "all"),
    "superseded_a": (2, "all"), "superseded_b": (1, 5), "during_init": (1, "all"), "big_yaw": (1, "all"), "bound": (2, "all"), "td": (6, "all"),
    "w11": (6, "all"), "w20": (12, "all"),
}


@pytest.mark.parametrize("name", RC.PARITY_CASES)
def test_case_latches_carries_its_factors_and_is_consumed_by_exactly_one_solve(P, orc, name):
    case, run = _run(P, name)
    fr, reqs = run["frames"], run["requests"]
    W, sf = case.cfg.window_size, RC.solve_frame(case)
    local, nf = EXPECT[name]
    assert len(fr) <= 40 and len(reqs) == len(case.requests) and len(fr) - sf > 4         # at least four frames follow the relocalisation solve
    assert [int(r["status"]["solver_flag"]) for r in fr] == [0] * W + [1] * (len(fr) - W)
    assert all(int(r["status"]["reboot_count"]) == 0 for r in fr)
    # the latch: pending from the request on, with the slot the request named (an unknown stamp leaves the earlier latch alone)
    for rq, q in zip(case.requests, reqs):
        assert q["relo"]["pending"] == 1 and q["relo"]["local_index"] == (rq.index if not rq.unknown else reqs[0]["relo"]["local_index"]), name
        stamp = q["args"][0]
        assert (stamp in fr[rq.after]["window"][:W, 16].tolist()) == (not rq.unknown)
    assert reqs[-1]["relo"]["local_index"] == local
    # consumed by exactly one solve: pending before it, the factors in it, none after it
    for k in range(case.requests[-1].after + 1, len(fr)):
        r = fr[k]["relo"]
        assert r["pending"] == (1 if k < sf else 0), (k, r["pending"])
        assert r["local_index"] == local
        if k != sf:
            assert r["n_factors"] == 0, (k, r["n_factors"])
    rs, ss = fr[sf]["relo"], fr[sf]["status"]
    want = int(ss["n_in_problem"]) if nf == "all" else nf
    if nf is not None:
        assert rs["n_factors"] == want, (rs["n_factors"], want)
    assert 1 <= ss["iterations"] <= case.cfg.max_iterations
    assert np.isfinite(ss["final_cost"]) and ss["final_cost"] <= ss["initial_cost"]
    for r in fr:
        assert np.all(np.isfinite(r["window"])) and all(np.all(np.isfinite(np.asarray(v, np.float64))) for v in r["relo"].values())
    dr = rs["drift_r"]
    assert abs(np.linalg.det(dr) - 1) < 1e-12 and abs(dr[2, 2] - 1) < 1e-12            # a pure yaw rotation
    assert abs(np.linalg.norm(rs["relative_q"]) - 1) < 1e-12


def test_the_start_filter_bites_at_index_0(P, orc):
    """slot 0: its old frame lies outside the window, and the in-problem landmarks that start in slot 1 are no factors"""
    c0, r0 = _run(P, "index_0")
    c1, r1 = _run(P, "index_1")
    sf = RC.solve_frame(c0)
    n0, n1 = r0["frames"][sf]["relo"]["n_factors"], r1["frames"][sf]["relo"]["n_factors"]
    assert 0 < n0 < n1 == int(r1["frames"][sf]["status"]["n_in_problem"]), (n0, n1)
    lm = r0["frames"][sf - 1]["lm"]
    late = int(np.count_nonzero(RC.in_problem_rows(lm, c0.cfg.window_size) & (lm[:, 1] == 1)))
    assert late >= 1 and n1 - n0 == late
    k = c0.requests[0].after
    old = int(np.argmin(np.abs(c0.stream.stamps - r0["requests"][0]["args"][0]))) - c0.requests[0].back
    assert c0.stream.stamps[old] < r0["frames"][k]["window"][0, 16]


def test_zero_one_and_two_factor_requests_are_what_they_claim(P, orc):
    case, run = _run(P, "no_overlap")
    mp = run["requests"][0]["args"][2]
    assert len(mp) > 60 and mp[:, 2].min() > case.stream.next_id
    assert _run(P, "empty")[1]["requests"][0]["args"][2] is None
    case, run = _run(P, "single")
    assert len(run["requests"][0]["args"][2]) == 1
    case, run = _run(P, "not_in_problem")
    k, mp = case.requests[0].after, run["requests"][0]["args"][2]
    lm, W = run["frames"][k]["lm"], case.cfg.window_size
    rows = {int(r[0]): r for r in lm}
    assert len(mp) >= 4 and all(int(i) in rows for i in mp[:, 2])                      # every id is in the table ...
    inp = {int(r[0]) for r in lm[RC.in_problem_rows(lm, W)]}
    kinds = {("late" if int(i) in inp else "out") for i in mp[:, 2]}
    assert kinds == {"late", "out"}                                                     # ... in problem but starting after slot 0, or not in problem
    assert all(rows[int(i)][1] > 0 for i in mp[:, 2] if int(i) in inp)
    case, run = _run(P, "ends")
    mp = run["requests"][0]["args"][2]
    lm = run["frames"][case.requests[0].after]["lm"]
    ids = set(lm[:, 0].astype(int).tolist())
    assert len(mp) == BC.tracker_capacity(case.cfg) and np.all(np.diff(mp[:, 2]) > 0)
    assert [int(i) in ids for i in mp[:, 2]] == [True] + [False] * (len(mp) - 2) + [True]


def test_the_copied_pose_after_a_keyframe_and_after_a_non_keyframe(P, orc):
    """setReloFrame copies para_Pose[i] as the last vector2double left it (relo_pose right after the request): after a MARGIN_OLD frame that is
    the pre-slide window, so the copy is the pose of slot i - 1; after the first non-keyframe of a hold it is slot i exactly; after the second,
    slot i as the solve left it, short of the gauge fix"""
    case, run = _run(P, "after_keyframe")
    q, k = run["requests"][0], case.requests[0].after
    w = run["frames"][k]["window"]
    assert int(run["frames"][k]["status"]["marginalization_flag"]) == 0
    assert _dist(q["relo"]["relo_pose"][:3], w[1, :3]) > 0.05 and _dist(q["relo"]["relo_pose"][:3], w[0, :3]) == 0.0
    case, run = _run(P, "after_non_keyframe")
    q, k = run["requests"][0], case.requests[0].after
    w = run["frames"][k]["window"]
    assert int(run["frames"][k]["status"]["marginalization_flag"]) == 1 and int(run["frames"][k - 1]["status"]["marginalization_flag"]) == 0
    assert _dist(q["relo"]["relo_pose"][:3], w[1, :3]) == 0.0
    assert _dist(q["relo"]["relo_pose"][3:7], w[1, [4, 5, 6, 3]]) < 1e-15               # (window: q as w x y z; relo_pose: x y z w)
    case, run = _run(P, "after_second_non_keyframe")
    q, k = run["requests"][0], case.requests[0].after
    assert int(run["frames"][k]["status"]["marginalization_flag"]) == 1 and int(run["frames"][k - 1]["status"]["marginalization_flag"]) == 1
    assert 0.0 < _dist(q["relo"]["relo_pose"][:3], run["frames"][k]["window"][1, :3]) < 1e-3


def test_superseded_requests(P, orc):
    """(a) the later index, match points and pose win; (b) an unknown stamp leaves the latch and the copied pose alone but replaces match
    points, count and the old keyframe's pose (upstream assigns them before it looks the stamp up)"""
    case, run = _run(P, "superseded_a")
    only2 = RC.Case("second_alone", case.stream, case.requests[1:], "")
    alone = RC.drive(only2, RC.oracle_accessors(), resolved=[run["requests"][1]["args"]])
    sf = RC.solve_frame(case)
    for key, v in run["frames"][sf]["relo"].items():
        assert np.array_equal(np.asarray(v), np.asarray(alone["frames"][sf]["relo"][key])), key     # as if the first had never been made
    assert _dist(run["requests"][0]["relo"]["relo_pose"], run["requests"][1]["relo"]["relo_pose"]) > 0.05
    case, run = _run(P, "superseded_b")
    a, b = run["requests"]
    assert b["args"][0] == RC.UNKNOWN_STAMP and np.array_equal(a["relo"]["relo_pose"], b["relo"]["relo_pose"]) and b["relo"]["local_index"] == 1
    sf = RC.solve_frame(case)
    assert run["frames"][sf]["relo"]["n_factors"] == len(b["args"][2]) == 5 < len(a["args"][2])
    # the drift is measured against the SECOND request's pose: against index_1 (the first request alone) the outputs differ
    first = _run(P, "index_1")[1]["frames"][sf]["relo"]
    assert _dist(first["drift_t"], run["frames"][sf]["relo"]["drift_t"]) > 1e-6


def test_during_init_waits_for_the_solve_that_ends_the_initialisation(P, orc):
    case, run = _run(P, "during_init")
    k, W = case.requests[0].after, case.cfg.window_size
    assert k + 1 < W and int(run["frames"][k]["status"]["solver_flag"]) == 0
    assert [run["frames"][f]["relo"]["pending"] for f in range(k + 1, W + 1)] == [1] * (W - k - 1) + [0]
    assert np.array_equal(run["requests"][0]["relo"]["relo_pose"], [0, 0, 0, 0, 0, 0, 1])   # para_Pose before the first solve: identity poses


def test_big_yaw_turns_the_drift_correction_by_its_angle(P, orc):
    case, run = _run(P, "big_yaw")
    sf = RC.solve_frame(case)
    big, ref = run["frames"][sf]["relo"], _run(P, "index_1")[1]["frames"][sf]["relo"]
    yaw = np.degrees(np.arctan2(big["drift_r"][1, 0], big["drift_r"][0, 0]))
    assert 178.0 < abs(yaw) <= 180.0, yaw
    a = np.radians(case.requests[0].yaw_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    assert _dist(big["drift_r"], Rz @ ref["drift_r"]) < 1e-9 and _dist(big["drift_t"], Rz @ ref["drift_t"]) < 1e-9
    for key in ("relative_t", "relative_q", "relative_yaw", "relo_pose"):                # the solve itself does not see the old keyframe's pose
        assert np.array_equal(np.asarray(big[key]), np.asarray(ref[key])), key


def test_bound_runs_the_line_search_inside_the_relocalisation_solve(P, orc):
    case, run = _run(P, "bound")
    sf = RC.solve_frame(case)
    (e0, _), (e1, _) = run["frames"][sf - 1]["line_search"], run["frames"][sf]["line_search"]
    (_, b0), (_, b1) = run["frames"][sf - 1]["bounds"], run["frames"][sf]["bounds"]
    assert e1 - e0 >= 1 and b1 - b0 >= 1, (e0, e1, b0, b1)
    assert run["frames"][sf]["relo"]["n_factors"] >= 40


def test_td_is_active_before_and_in_the_relocalisation_solve(P, orc):
    case, run = _run(P, "td")
    sf = RC.solve_frame(case)
    td = [float(r["status"]["td"]) for r in run["frames"]]
    assert (case.cfg.window_size, case.cfg.estimate_td, case.cfg.estimate_extrinsic) == (10, 1, 0)
    assert td[sf - 3] != td[sf - 2] != td[sf - 1] != td[sf] and abs(td[sf]) < 0.05


@pytest.mark.parametrize("name,W,tol", [("w11", 11, 1e-3), ("w20", 20, 1e-4)])
def test_wide_windows_relocalise_onto_the_truth(P, orc, name, W, tol):
    case, run = _run(P, name)
    assert case.cfg.window_size == W
    sf, rq = RC.solve_frame(case), case.requests[0]
    stamp, _, mp, p_k, R_k = run["requests"][0]["args"]
    p_i = case.stream.scene.pose(stamp)[0]
    assert run["frames"][sf]["relo"]["n_factors"] == len(mp) == 49
    assert _dist(run["frames"][sf]["relo"]["relative_t"], R_k.T @ (p_i - p_k)) < tol


def test_vo_request_latches_on_the_literal_oracle(P, orc):
    """the reference has no use_imu test in setReloFrame or in the factor loop: the oracle carries the factors in VO mode and consumes the request;
    the HIP path drops it instead (overflow bit 64), which test_gpu_relo_edges checks against a twin handle"""
    case, run = _run(P, "vo")
    assert case.cfg.use_imu == 0
    q, sf = run["requests"][0], RC.solve_frame(case)
    assert q["relo"]["pending"] == 1 and q["relo"]["local_index"] == 1
    assert q["args"][0] in run["frames"][case.requests[0].after]["window"][:case.cfg.window_size, 16].tolist()
    assert run["frames"][sf]["relo"]["pending"] == 0 and run["frames"][sf]["relo"]["n_factors"] > 0
