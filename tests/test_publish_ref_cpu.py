"""The batched publishers (vio_publish_all): what can be checked without a GPU.  The numpy definition the GPU tests use
(publish_ref.py) on hand-made tables that sit on both sides of every comparison it makes, the oracle over the streams of publish_cases.py to
show that between them they take every branch of the definition a live estimator can take, and the library's exports and argument checks."""
import numpy as np
import pytest

import publish_cases as PC
import publish_ref as PR
import vio_ct

VIO_EINVAL = -1
# setDepth marks a landmark whose solved depth is negative with solve_flag 2 and removeFailures erases it before processImage returns
# (estimator.cpp: slideWindow(); f_manager.removeFailures();): no publisher ever sees the value on a live estimator.  The hand-made tables and
# the stage tests hold it; the stream test asserts that it never shows up, so that this note cannot go stale.
UNREACHABLE_LIVE = {"solve_flag=2"}


def table(W, rows):
    """rows of (id, start, n_obs, solve_flag, is_dynamic, depth0): landmarks_ex rows with estimated depth 2 + id / 8 and the first observation
    at (0.01 id, -0.02 id, 1); the window: P = (f, 2 f, 3 f), a rotation about z by 0.1 f, stamp 100 + f"""
    lm = np.array([[i, s, n, 2.0 + i / 8.0, 1, sf, dy, 0.01 * i, -0.02 * i, 1.0, d0, 0.0] for i, s, n, sf, dy, d0 in rows], np.float64).reshape(-1, 12)
    win = np.zeros((W + 1, 17))
    for f in range(W + 1):
        win[f, 0:3] = (f, 2 * f, 3 * f)
        win[f, 3:7] = (np.cos(0.05 * f), 0, 0, np.sin(0.05 * f))
        win[f, 16] = 100.0 + f
    ex = np.concatenate([[0.1, 0.2, 0.3], np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64).reshape(-1), [0.0]])
    fed = {100.0 + W - 2: {int(r[0]): np.array([0.5 + r[0], 0.25 + r[0], 1.0, 10.0 + r[0], 20.0 + r[0], 0, 0]) for r in rows}}
    return lm, win, ex, fed


NONLINEAR = dict(solver_flag=1, marginalization_flag=0, processed=1)


def ids(rows):
    return [int(v) for v in rows[:, 7]]


def run(W, rows, status=NONLINEAR):
    lm, win, ex, fed = table(W, rows)
    counts, pose, cloud, margin, kf = PR.publish(lm, win, ex, status, fed)
    assert (counts[0], counts[1], counts[2]) == (len(cloud), len(margin), len(kf))
    return counts, pose, cloud, margin, kf


def cloud_ids(W, rows, which, status=NONLINEAR):
    """the ids behind a list: every row is published with a distinct point, so the list is identified by running the rows one at a time"""
    out = []
    for r in rows:
        got = run(W, [r], status)[which]
        assert len(got) in (0, 1)
        if len(got):
            out.append(r[0])
    full = run(W, rows, status)[which]
    assert len(full) == len(out)
    return out


def test_n_obs_and_start_sit_on_both_sides_of_the_cloud_tests():
    W = 10
    rows = [(1, 0, 1, 1, 0, 1.5), (2, 0, 2, 1, 0, 1.5), (3, 0, 3, 1, 0, 1.5),          # n_obs 1 / 2 / 3
            (4, W - 3, 2, 1, 0, 1.5), (5, W - 2, 2, 1, 0, 1.5)]                           # start W-3 / W-2
    assert cloud_ids(W, rows, 2) == [2, 3, 4]
    assert cloud_ids(W, rows, 3) == [2]                                                   # margin: start 0 and n_obs <= 2
    assert cloud_ids(W, [(6, 1, 2, 1, 0, 1.5)], 3) == []                                  # ... start 1 is out


def test_three_quarters_of_the_window_bites_at_20_and_cannot_at_10():
    assert cloud_ids(20, [(1, 15, 2, 1, 0, 1.0), (2, 16, 2, 1, 0, 1.0), (3, 17, 2, 1, 0, 1.0), (4, 18, 2, 1, 0, 1.0)], 2) == [1]
    # W = 10: start < W - 2 = 8 leaves 7 as the largest start, and 7 > 7.5 is false
    assert cloud_ids(10, [(1, 7, 2, 1, 0, 1.0), (2, 8, 2, 1, 0, 1.0)], 2) == [1]
    # the keyframe list has no such test
    assert cloud_ids(20, [(1, 15, 4, 1, 0, 1.0), (2, 16, 3, 1, 0, 1.0), (3, 17, 2, 1, 0, 1.0), (4, 18, 2, 1, 0, 1.0)], 4) == [1, 2, 3]


def test_solve_flag_and_is_dynamic():
    W = 10
    rows = [(1, 0, 2, 0, 0, 1.0), (2, 0, 2, 1, 0, 1.0), (3, 0, 2, 2, 0, 1.0), (4, 0, 9, 1, 1, 1.0), (5, 0, 9, 0, 1, 1.0)]
    assert cloud_ids(W, rows, 2) == [2]
    assert cloud_ids(W, rows, 3) == [2]
    assert cloud_ids(W, rows, 4) == [4]          # dynamic: in neither cloud, in the keyframe; solve_flag 1 only


def test_a_zero_depth_falls_back_to_the_estimated_depth():
    W = 10
    a, b = run(W, [(8, 2, 3, 1, 0, 0.0)])[2], run(W, [(8, 2, 3, 1, 0, 3.0)])[2]
    # estimated depth 2 + 8 / 8 = 3: the same point either way, and another one for another depth
    assert np.array_equal(a, b) and not np.array_equal(a, run(W, [(8, 2, 3, 1, 0, 3.5)])[2])
    # the point itself: pc = (0.08, -0.16, 1) * 3; ric = rot z 90: pi = (-pc.y, pc.x, pc.z) + tic; R(0.2 rad about z), P = (2, 4, 6)
    pc = np.array([0.08, -0.16, 1.0]) * 3.0
    pi = np.array([-pc[1], pc[0], pc[2]]) + [0.1, 0.2, 0.3]
    c, s = np.cos(0.2), np.sin(0.2)
    want = np.array([c * pi[0] - s * pi[1], s * pi[0] + c * pi[1], pi[2]]) + [2, 4, 6]
    assert np.abs(a[0] - want).max() < 1e-14


def test_the_keyframe_needs_the_track_to_reach_frame_w_minus_2_and_all_three_conditions():
    W = 10
    rows = [(1, 0, W - 2, 1, 0, 1.0), (2, 0, W - 1, 1, 0, 1.0),        # start + n_obs - 1 = W-3 / W-2
            (3, W - 3, 2, 1, 0, 1.0), (4, W - 2, 3, 1, 0, 1.0)]        # start W-3 / W-2
    counts, pose, _, _, kf = run(W, rows)
    assert ids(kf) == [2, 3] and counts[3] == 1
    lm, win, ex, fed = table(W, rows)
    assert np.array_equal(pose, np.concatenate([[win[W - 2, 16]], win[W - 2, 0:3], win[W - 2, 3:7]]))
    assert np.array_equal(kf[0, 3:7], [2.5, 2.25, 12.0, 22.0])        # x, y, u, v of the observation filed under frame W-2
    for off in (dict(solver_flag=0), dict(marginalization_flag=1), dict(processed=0)):
        counts, pose, cloud, margin, kf = run(W, rows, dict(NONLINEAR, **off))
        assert pose is None and len(kf) == 0 and (counts[2], counts[3]) == (0, 0), off
        assert len(cloud) == 3                                          # the clouds do not look at the status (start W-2 alone is out)


def test_the_streams_take_every_branch_a_live_estimator_can_take(P):
    taken, per = set(), {}
    seen = dict(margin=0, second_new=0, initial=0, unprocessed=0)
    for name in PC.STREAMS:
        tk = set()
        recs = PC.run_oracle(PC.build(name, P), tk)
        per[name], taken = tk, taken | tk
        for r in recs:
            seen["margin"] += int(r["out"][0][1] > 0)
            seen["second_new"] += int(r["status"]["solver_flag"] == 1 and r["status"]["marginalization_flag"] == 1)
            seen["initial"] += int(r["status"]["solver_flag"] == 0)
            seen["unprocessed"] += int(not r["processed"])
    for b in PR.BRANCHES:
        print("%-26s %s" % (b, " ".join(n for n in PC.STREAMS if b in per[n]) or "-"))
    assert not (set(PR.BRANCHES) - UNREACHABLE_LIVE - taken), sorted(set(PR.BRANCHES) - UNREACHABLE_LIVE - taken)
    assert not (UNREACHABLE_LIVE & taken)
    assert all(v > 0 for v in seen.values()), seen


def test_the_track_mirror_is_the_fed_map_where_no_track_has_a_gap(P):
    """on a stream without returning ids or skipped depths the observation filed under window frame W-2 is the one fed at that stamp"""
    st = PC.build("short_tracks", P)
    W = st.cfg.window_size
    by_stamp = {float(f[0]): dict(zip((int(i) for i in f[1]), f[2])) for f in st.frames()}
    n = 0
    for r in PC.run_oracle(st):
        for q in r["out"][4]:
            o = by_stamp[float(r["window"][W - 2, 16])][int(q[7])]
            assert np.array_equal(q[3:7], [o[0], o[1], o[3], o[4]])
            n += 1
    assert n > 100


def test_the_publishers_are_exported(P):
    L = P.lib()
    for name in ("vio_publish_all", "vio_stage_publish"):
        assert hasattr(L, name), name
    assert hasattr(P.VioBatch, "publish") and hasattr(P, "stage_publish") and P.PUBLISH_BLOCK == 256
    assert L.vio_abi_version() == 12


def test_bad_arguments_are_refused(P):
    L = P.lib()
    c = np.zeros(4, np.int32)
    assert L.vio_publish_all(None, 4, c.ctypes.data, None, None, None, None, 0) == VIO_EINVAL
    W, NL = 4, 8
    t = dict(lm_order=np.arange(NL), lm_id=np.arange(NL), lm_start=np.zeros(NL), lm_nobs=np.zeros(NL), lm_solve_flag=np.zeros(NL),
             lm_dyn=np.zeros(NL), lm_depth=np.ones(NL), lm_obs=np.zeros((NL, W + 1, 9)), Ps=np.zeros((W + 1, 3)), Rs=np.zeros((W + 1, 9)),
             Headers=np.zeros(W + 1), ric=np.eye(3), tic=np.zeros(3))
    with pytest.raises(ValueError):
        P.stage_publish(t, W, 0, 0, (1, 0, 1), -1)
    with pytest.raises(ValueError):
        P.stage_publish(t, 1, 0, 0, (1, 0, 1), 4)
    with pytest.raises(ValueError):
        P.stage_publish(dict(t, lm_obs=np.zeros((NL, W, 9))), W, 0, 0, (1, 0, 1), 4)
    with pytest.raises(ValueError):
        P.stage_publish(t, W, 0, 0, (1, 0), 4)
    with pytest.raises(KeyError):
        P.stage_publish({k: v for k, v in t.items() if k != "tic"}, W, 0, 0, (1, 0, 1), 4)
    # the C entry checks for itself
    f = np.array([1, 0, 1], np.int32)
    pose = np.zeros(8)
    assert L.vio_stage_publish(NL, W, 0, 0, None, f.ctypes.data, 0, c.ctypes.data, pose.ctypes.data, None, None, None) == VIO_EINVAL
    pt = P.PublishTables()
    assert L.vio_stage_publish(NL, W, 0, 0, pt, f.ctypes.data, 0, c.ctypes.data, pose.ctypes.data, None, None, None) == VIO_EINVAL


def test_replay_takes_the_two_output_options_and_the_writer_slices_by_the_counts(tmp_path):
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(vio_ct.ROOT, "tools"))
    import replay
    a, _ = replay.parse_args(["--config", "c.yaml", "--data", "d", "--keyframes-out", "kf", "--cloud-out", "c.npz"])
    assert (a.keyframes_out, a.cloud_out) == ("kf", "c.npz")
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")

    class Fake:
        S = 2

        def publish(self, lists):
            assert lists == (True, True, True)
            return dict(counts=np.array([[2, 1, 3, 1], [1, 0, 0, 0]], np.int32), kf_pose=np.arange(16.0).reshape(2, 8) + 0.5,
                        cloud=np.arange(24.0).reshape(2, 4, 3), margin=-np.arange(24.0).reshape(2, 4, 3), kf_points=np.arange(64.0).reshape(2, 4, 8))
    pw = io.PublicationWriter(str(tmp_path / "kf"), str(tmp_path / "c.npz"))
    pw.poll(Fake(), [0, 1])
    pw.poll(Fake(), [])
    pw.close()
    assert pw.n_keyframes == 1 and os.listdir(str(tmp_path / "kf")) == ["kf_0_500000000.npz"]
    z = np.load(str(tmp_path / "kf" / "kf_0_500000000.npz"))
    assert np.array_equal(z["pose"], np.arange(8.0) + 0.5) and z["points"].shape == (3, 8)
    c = np.load(str(tmp_path / "c.npz"))
    assert c["cloud_0"].shape == (2, 3) and c["margin_0"].shape == (1, 3) and c["cloud_1"].shape == (1, 3) and c["margin_1"].shape == (0, 3)
