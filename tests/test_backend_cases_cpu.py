"""The generated back-end streams (tests/backend_cases.py) checked on the CPU: the generator's geometry against an independent projection,
and, on the oracle alone, that every case initialises, never reboots and REACHES the branch it is named for -- so that the GPU comparison of
tests/test_gpu_backend_edges.py cannot pass vacuously.

On convergence.  The reference gives a solve NUM_ITERATIONS = 8 trust-region iterations, and that budget, not a tolerance, ends 24 % of the
solves of the rendered scene (tests/golden/oracle_decisions_300.npz).  The generated streams are harder on it: a 4-frame window holds only
the landmarks that start in its first two frames, the frames are 0.2 - 1 s apart, depths are quantised to millimetres.  Most of their solves on
moving frames therefore end on the budget; documented here for every case.  What is asserted instead: every solve leaves the cost finite and
no higher than it found it, and the solves of the long standstill, where nothing moves, do stop by tolerance."""
import numpy as np
import pytest

import backend_cases as BC
import excalib_ref as X

_runs = {}


def _run(P, name):
    if name not in _runs:
        _runs[name] = (BC.build(name, P), BC.run_oracle(BC.build(name, P)))
    return _runs[name]


def _flags(recs, key):
    return [int(r["status"][key]) for r in recs]


# ------------------------------------------------------------------------------------------------------------- generator
def test_generated_observations_reproject_and_depth_holds_the_landmark_depths(P):
    """standstill_short publishes landmark j under id j: every observation against a projection written out here (not CaseScene.project), the
    depth image at the observation's pixel, the velocity columns as the difference quotient of consecutive frames"""
    st = BC.build("standstill_short", P)
    sc, cfg = st.scene, st.cfg
    prev = None
    for stamp, ids, obs, depth, _ in st.frames():
        p, R = sc.pose(stamp)
        Rwc, pwc = R @ X.RIC_TRUE, p + R @ X.TIC_TRUE
        assert len(ids) >= 45 and np.all(np.diff(ids) > 0)
        for fid, o in zip(ids, obs):
            Pc = Rwc.T @ (sc.L[fid] - pwc)
            assert abs(o[0] - Pc[0] / Pc[2]) < 1e-12 and abs(o[1] - Pc[1] / Pc[2]) < 1e-12 and o[2] == 1.0
            assert abs(o[3] - (cfg.fx * Pc[0] / Pc[2] + cfg.cx)) < 1e-9 and abs(o[4] - (cfg.fy * Pc[1] / Pc[2] + cfg.cy)) < 1e-9
            assert 0 <= o[3] < cfg.width and 0 <= o[4] < cfg.height
            assert abs(int(depth[int(o[4]), int(o[3])]) - Pc[2] * 1000.0) <= 0.5
            if prev is not None and fid in prev[1]:
                assert np.abs(o[5:7] - (o[0:2] - prev[1][fid]) / (stamp - prev[0])).max() < 1e-12
        assert np.count_nonzero(depth) == len(ids)       # nothing else in the image
        prev = (stamp, {int(f): o[0:2].copy() for f, o in zip(ids, obs)})


def test_generated_imu_is_gravity_alone_while_the_rig_holds_still_and_integrates_to_the_path(P):
    st = BC.build("standstill_short", P)
    sc, W = st.scene, st.cfg.window_size
    ts, acc, gyr = sc.imu(st.stamps[-1] + 1.0)
    hold = (ts > st.stamps[W + 5]) & (ts < st.stamps[W + 4 + 12])
    assert hold.sum() > 100
    assert np.abs(gyr[hold]).max() == 0.0 and np.abs(np.linalg.norm(acc[hold], axis=1) - st.cfg.g_norm).max() < 1e-6
    # the pushed slices are the samples in order, none lost, each reaching past its frame's stamp
    k = 0
    for stamp, _, _, _, (ti, ai, gi) in st.frames():
        assert np.array_equal(ti, ts[k:k + len(ti)]) and np.array_equal(ai, acc[k:k + len(ti)]) and ti[-1] >= stamp
        k += len(ti)
    # midpoint integration of the samples over the first move reproduces the analytic displacement (50 Hz: a few mm)
    a, b = np.searchsorted(ts, st.stamps[W]), np.searchsorted(ts, st.stamps[W + 4])
    p, R = sc.pose(ts[a])
    v, g = np.zeros(3), np.array([0, 0, st.cfg.g_norm])
    for q in range(a, b):
        dt = ts[q + 1] - ts[q]
        R1 = R @ X.rodrigues(0.5 * (gyr[q] + gyr[q + 1]) * dt)
        aw = 0.5 * (R @ acc[q] + R1 @ acc[q + 1]) - g
        p, v, R = p + v * dt + 0.5 * aw * dt * dt, v + aw * dt, R1
    pe, Re = sc.pose(ts[b])
    assert np.abs(p - pe).max() < 0.01 and X.rot_angle_deg(R, Re) < 0.05 and np.linalg.norm(pe) > 0.3


def test_capacity_formulas_and_the_hash_chain(P):
    cfg = BC.case_config(P)
    assert (BC.tracker_capacity(cfg), BC.landmark_capacity(cfg)) == (96, 200) and BC.lm_hash_size(200) == 512 and BC.lm_hash_size(96) == 256
    assert BC.landmark_capacity(BC.build("table_full", P).cfg) == 96
    st = BC.build("hash_chain", P)
    ht, chain = st.notes["ht"], st.notes["chain"]
    assert ht == BC.lm_hash_size(BC.landmark_capacity(st.cfg)) and len(chain) >= 24
    assert {BC.hash_bucket(i, ht) for i in chain} == {ht - 3}           # one bucket, and the probe chain wraps round the table's end
    assert len({(i - chain[0]) % ht for i in chain}) == 1
    seen = set()
    for k, (_, ids, _, _, _) in enumerate(st.frames()):
        assert set(chain) <= set(ids.tolist()) and BC.INT32_MAX - 1 in ids and 0 in ids and ids.min() >= 0
        assert not np.all(np.diff(ids) > 0)
        seen.add(tuple(ids.tolist()))
    assert len(seen) == len(st.frames())                                # another order every frame


# ------------------------------------------------------------------------------------------------------------- the oracle on every case
@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_initialises_on_frame_w_never_reboots_and_every_solve_descends(P, orc, name):
    st, recs = _run(P, name)
    W = st.cfg.window_size
    assert len(recs) <= 40
    assert _flags(recs, "solver_flag") == [0] * W + [1] * (len(recs) - W)
    assert all(r["rc"] == 1 for r in recs) and _flags(recs, "reboot_count") == [0] * len(recs)
    assert _flags(recs, "frames_processed") == list(range(1, len(recs) + 1))
    counts = st.imu_counts()
    assert max(counts[1:]) <= (65 if name == "imu_65" else BC.IMU_SLOT_CAP)
    for k, r in enumerate(recs[W:], W):
        s = r["status"]
        assert 1 <= s["iterations"] <= st.cfg.max_iterations, k
        assert np.isfinite(s["final_cost"]) and s["final_cost"] <= s["initial_cost"], (k, s["initial_cost"], s["final_cost"])
        assert np.all(np.isfinite(r["window"]))


def _standstill_conditions(st, recs, W):
    slots = [BC.long_interval_slot(r["window"], W) for r in recs]
    flags = _flags(recs, "marginalization_flag")
    first = slots.index(W - 1)
    assert first > W + 10 and max(slots[:first]) == 0
    # while it sits in slot W - 1 every frame is a non-keyframe merged into it, and the solves there see an interval > 10 s
    assert all(flags[k] == 1 for k in range(first - 5, first + 1))
    # then it slides down one slot per keyframe; with it in slot 1 the next frame marginalises frame 0 (MARGIN_OLD) without its IMU factor
    at1 = [k for k in range(len(recs) - 1) if slots[k] == 1]
    assert at1 and flags[at1[-1] + 1] == 0 and slots[at1[-1] + 1] == 0
    assert [s for k, s in enumerate(slots[first:]) if k == 0 or s != slots[first + k - 1]] == list(range(W - 1, -1, -1))
    return first, at1[-1] + 1


def test_standstill_reaches_an_interval_beyond_ten_seconds_and_marginalises_it(P, orc):
    st, recs = _run(P, "standstill")
    W = st.cfg.window_size
    first, marg = _standstill_conditions(st, recs, W)
    assert len(recs) - marg >= 3                                       # the sequence goes on after that marginalisation
    its = _flags(recs, "iterations")
    assert sum(1 for k in range(W + 8, first) if its[k] < st.cfg.max_iterations) >= 10     # the standstill's solves stop by tolerance


def test_standstill_short_stays_below_ten_seconds(P, orc):
    st, recs = _run(P, "standstill_short")
    W = st.cfg.window_size
    assert all(BC.long_interval_slot(r["window"], W) == 0 for r in recs)
    assert max(BC.long_interval_slot(r["window"], W, 6.0) for r in recs) == W - 1     # the same merges, to 7 s
    h = np.array([r["window"][:W, 16] for r in recs])
    assert 6.0 < np.diff(h, axis=1).max() < 10.0
    at1 = [k for k in range(len(recs) - 1) if BC.long_interval_slot(recs[k]["window"], W, 6.0) == 1]
    assert at1 and _flags(recs, "marginalization_flag")[at1[-1] + 1] == 0           # and the same MARGIN_OLD, with its factor


def test_w10_td_reaches_the_same_branches_with_td_and_extrinsic_estimated(P, orc):
    st, recs = _run(P, "w10_td")
    assert (st.cfg.window_size, st.cfg.estimate_td, st.cfg.estimate_extrinsic) == (10, 1, 1)
    _standstill_conditions(st, recs, 10)
    assert abs(recs[-1]["status"]["td"]) > 0 and all(abs(r["status"]["td"]) < 0.05 for r in recs)


def test_imu_counts_puts_every_count_on_a_keyframe_and_on_a_non_keyframe(P, orc):
    st, recs = _run(P, "imu_counts")
    W = st.cfg.window_size
    counts, flags = st.imu_counts(), _flags(recs, "marginalization_flag")
    assert counts[W + 3:-2] == [c for c in BC.IMU_COUNTS for _ in (0, 1)]
    assert set(counts[1:W + 3] + counts[-2:]) == {21}
    seen = {(counts[k], flags[k]) for k in range(W + 1, len(recs))}
    for c in BC.IMU_COUNTS:
        assert (c, 0) in seen and (c, 1) in seen, c                      # 0: new-frame propagation only; 1: also merged into slot W - 1
    assert {c % BC.PI_CH for c in BC.IMU_COUNTS} >= {0, 1, 7} and max(BC.IMU_COUNTS) == BC.IMU_SLOT_CAP
    assert len(set(st.stamps.tolist())) == len(st.stamps) and np.all(np.diff(st.stamps) > 0)


def test_imu_65_is_one_non_keyframe_with_65_samples(P, orc):
    st, recs = _run(P, "imu_65")
    counts, f = st.imu_counts(), st.notes["overflow_frame"]
    assert counts[f] == BC.IMU_SLOT_CAP + 1 and max(counts[1:f] + counts[f + 1:]) == 21
    assert _flags(recs, "marginalization_flag")[f] == 1 and len(recs) - f > st.cfg.window_size


def test_thin_exercises_the_three_keyframe_rules(P, orc):
    st, recs = _run(P, "thin")
    W, n = st.cfg.window_size, st.notes
    trk, flags = _flags(recs, "last_track_num"), _flags(recs, "marginalization_flag")
    full = len(st.frames()[n["f_pnum0"]][1])
    assert (trk[n["f19"]], flags[n["f19"]]) == (19, 0)                   # fewer than 20 tracked: a keyframe whatever the parallax
    assert (trk[n["f20"]], flags[n["f20"]]) == (20, 1)                   # 20: the parallax rule decides, and says no here
    # pnum == 0: every feature of the frame is tracked, yet no landmark spans frames fc - 2 and fc - 1 (read off the table before the frame)
    lm = recs[n["f_pnum0"] - 1]["lm"]
    assert not np.any((lm[:, 1] <= W - 2) & (lm[:, 1] + lm[:, 2] - 1 >= W - 1))
    assert (trk[n["f_pnum0"]], flags[n["f_pnum0"]]) == (full, 0) and full >= 40
    assert len(st.frames()[n["f_single"]][1]) == 1 and flags[n["f_single"]] == 0


def test_table_full_fills_the_table_exactly(P, orc):
    st, recs = _run(P, "table_full")
    cap, n = BC.landmark_capacity(st.cfg), st.notes
    assert cap == BC.tracker_capacity(st.cfg) == 96
    nl = _flags(recs, "n_landmarks")
    assert nl[n["full_frame"]] == cap and max(nl[:n["full_frame"]]) < cap
    assert nl[n["overflow_frame"]] == cap + 1                              # the oracle's list is unbounded: one more than fits
    assert len(recs) - n["overflow_frame"] > st.cfg.window_size + 3


def test_short_tracks_has_one_two_and_three_observations_when_frame_0_leaves(P, orc):
    st, recs = _run(P, "short_tracks")
    W, n = st.cfg.window_size, st.notes
    ex = st.notes["extras"][n["f_short"]]
    k = n["f_short"] + W - 1                                            # the frame after which f_short is frame 0 of the window
    lm = recs[k]["lm"]
    rows = {int(r[0]): (int(r[1]), int(r[2])) for r in lm}
    assert [rows[i] for i in ex] == [(0, 1)] * 3 + [(0, 2)] * 3 + [(0, 3)] * 3
    assert _flags(recs, "marginalization_flag")[k + 1] == 0
    after = {int(r[0]): int(r[2]) for r in recs[k + 1]["lm"]}
    assert [after.get(i) for i in ex] == [None] * 6 + [2] * 3           # removeBackShiftDepth: fewer than 2 left -> erased
    for f in n["f_front"]:                                              # landmarks that start in frame W of a non-keyframe: removeFront moves them
        assert _flags(recs, "marginalization_flag")[f] == 1
        before, now = set(recs[f - 1]["lm"][:, 0].astype(int)), {int(r[0]): (int(r[1]), int(r[2])) for r in recs[f]["lm"]}
        new = st.notes["extras"][f]
        assert not set(new) & before and [now[i] for i in new] == [(W - 1, 1)] * len(new)


def test_reappear_re_appends_landmarks(P, orc):
    st, recs = _run(P, "reappear")
    fr = st.frames()
    gone = set(fr[8][1].tolist()) - set(fr[9][1].tolist())
    assert len(gone) == 8 and not gone & set(fr[10][1].tolist()) and gone <= set(fr[11][1].tolist())
    culled = set(int(st.ids_of[j]) for j in st.notes["culled"])
    assert all(culled <= set(f[1].tolist()) for f in fr[8:])            # their ids stay in the map throughout
    dyn = [int(r[6]) for r in recs[12]["lm"] if int(r[0]) in culled]
    assert dyn == [1] * len(culled)                                     # movingConsistencyCheck has marked every one of them, none was erased
    # removeFailures drops a returned landmark, and its id, still tracked, comes back at the end of the list: the list is no longer sorted by id
    order = [r["lm"][:, 0].astype(int).tolist() for r in recs]
    unsorted = [k for k, o in enumerate(order) if o != sorted(o)]
    assert unsorted and order[unsorted[0]][-1] in gone
    k = unsorted[0]
    assert order[k][-1] not in order[k - 1] and order[k][-1] in order[k - 2]


def test_depth_edges_skips_clamps_and_triangulates_without_depth(P, orc):
    st, recs = _run(P, "depth_edges")
    fr, cfg = st.frames(), st.cfg
    dmin, dmax = int(round(cfg.depth_min * 1000)), int(round(cfg.depth_max * 1000))
    px = lambda f, i: int(fr[f][3][min(max(int(fr[f][2][i, 4]), 0), cfg.height - 1), min(max(int(fr[f][2][i, 3]), 0), cfg.width - 1)])
    vals = {px(f, i) for f in range(7, 12) for i in range(len(fr[f][1]))}
    assert {0, dmin - 1, dmin, dmax + 1} <= vals
    # the skipped observation is not counted as tracked and its landmark gets no more observations
    assert _flags(recs, "last_track_num")[8] == len(fr[8][1]) - 1
    # pixel coordinates outside the image, and each finds its landmark's depth (the table's last-observation depth is the true one)
    uv = np.vstack([fr[f][2][:, 3:5] for f in (8, 9, 10)])
    assert {-0.5, float(cfg.width), cfg.width + 5.0} <= set(uv[:, 0].tolist()) and float(cfg.height) in set(uv[:, 1].tolist())
    rows = {int(r[0]): r for r in recs[9]["lm"]}
    for j in BC.EDGE_PIXELS:
        z = st.scene.project(fr[9][0])[2][j]
        assert abs(rows[j][11] - z) < 1e-3, (j, rows[j][11], z)                  # the oracle's unclamped index
        assert abs(px(9, fr[9][1].tolist().index(j)) / 1000.0 - z) < 1e-3, j    # the clamped look-up of the HIP path
    # depth-less triangulation: estimate_flag 2 (the DLT branch) on the landmark whose every observation lacks depth
    dl = int(st.ids_of[st.notes["depthless_lm"]])
    assert any(int(r[4]) == 2 and r[10] == 0 and r[11] == 0 for rec in recs for r in rec["lm"] if int(r[0]) == dl)
