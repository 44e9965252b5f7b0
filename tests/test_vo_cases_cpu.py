"""Every VO stream of backend_cases.VO_CASES reaches, on the oracle alone, the branch of FeatureManager::initFramePoseByPnP it is named for
(tests/test_gpu_pose_edges.py then compares the HIP back end with the oracle on them)."""
import numpy as np
import pytest

import backend_cases as BC

_runs = {}


def oracle_run(P, name):
    if name not in _runs:
        st = BC.build_vo(name, P)
        _runs[name] = (st, BC.run_oracle_vo(st))
    return _runs[name]


@pytest.mark.parametrize("name", list(BC.VO_CASES))
def test_vo_stream_initialises_and_solves_every_frame(P, name):
    st, out = oracle_run(P, name)
    W = st.cfg.window_size
    assert st.cfg.use_imu == 0      # (run_oracle_vo and the HIP runner push no IMU sample, whatever the stream carries)
    for k, r in enumerate(out):
        assert r["rc"] == 1 and int(r["status"]["solver_flag"]) == (1 if k >= W else 0), (name, k)
        assert r["pnp"][0] == (1 if k > W else 0), (name, k)      # solvePnP's turn comes on every frame after the initialisation
        assert np.abs(r["window"][:, 7:16]).max() == 0


def test_moving_start_frees_a_landmark_whose_first_step_is_a_rounding_residue(P, orc, tmp_path, monkeypatch):
    """vo_moving_start, the first VO solve: landmark 48 is free (the only variable landmark) with depth -1.  Under identical poses its
    projection does not depend on the depth: d r / d lambda is exactly 0 and comes out as a residue of 1e-13 whose size and sign change
    under an equivalent input (the extrinsic quaternion scaled by 1 + 3e-16), against 18 with a 0.1 m baseline; H_ll is 1e-28, the damping
    mu max(H_ll, 1e-6) = 1e-14 is all there is in the denominator, and the landmark's first step comes out of order 1"""
    import ctypes as C
    import excalib_ref as X
    import vio_ct
    st = BC.vo_moving_start(P)
    W = st.cfg.window_size
    fr = st.frames()

    def ob(k):
        o = fr[k][2][int(np.nonzero(fr[k][1] == 48)[0][0])]
        return np.array([o[0], o[1], o[2], o[3], o[4], o[5], o[6], 0.0, 4.5])

    def jl(pj, ex):
        r, J, pi = np.zeros(2), np.zeros(46), np.array([0, 0, 0, 0, 0, 0, 1.0])
        oi, oj = ob(0), ob(3)
        orc.ovio_eval_projection(C.byref(st.cfg), pi.ctypes.data, pj.ctypes.data, ex.ctypes.data, -1.0, 0.0, oi.ctypes.data, oj.ctypes.data, 0,
                                 r.ctypes.data, J.ctypes.data)
        return J[42:44].copy()
    q = X.R2q(X.RIC_TRUE)
    ex = np.r_[X.TIC_TRUE, q[1], q[2], q[3], q[0]]
    same = np.array([0, 0, 0, 0, 0, 0, 1.0])
    base = same.copy(); base[0] = 0.1
    ex_eq = ex.copy(); ex_eq[3:] *= 1 + 3e-16
    a, b = jl(same, ex), jl(same, ex_eq)
    assert np.abs(a).max() < 1e-11 and np.abs(b).max() < 1e-11 and np.abs(jl(base, ex)).min() > 1.0
    assert np.abs(a - b).max() > np.abs(a).max()            # the residue is not a property of the problem
    st.cfg.max_iterations = 1
    dump = tmp_path / "solve.bin"
    o = vio_ct.OraclePipeline(st.cfg)
    for k, (stamp, ids, obs, depth, _) in enumerate(fr[:W + 1]):
        if k == W:
            monkeypatch.setenv("OVIO_DUMP_SOLVE", str(dump))
        o.process_obs(ids, obs, BC.oracle_depth(depth), stamp)
    monkeypatch.delenv("OVIO_DUMP_SOLVE")
    d = np.fromfile(str(dump))
    Pa, Fa, mu = int(d[0]), int(d[1]), d[2]
    off = 4 + Pa * Pa + Fa * Pa
    Hll, dgl, gnl = d[off], d[off + Fa + Pa + Fa + Pa], d[off + Fa + Pa + Fa + Pa + Fa + Pa]
    lm = o.landmarks_ex()
    assert (Pa, Fa) == (6 * W, 1) and int(o.status()["n_var_landmarks"]) == 1 and lm[lm[:, 0] == 48][0][4] == 0
    assert Hll < 1e-24 and abs(mu * dgl * dgl - 1e-14) < 1e-20 and abs(gnl / dgl) > 1.0, (Hll, mu, dgl, gnl)


def test_few_pairs_counts(P):
    st, out = oracle_run(P, "vo_few_pairs")
    assert st.notes["pairs"] == {8: 5, 12: 4, 16: 3, 20: 0}
    for k, n in st.notes["pairs"].items():
        assert out[k]["pnp"][1] == n, (k, out[k]["pnp"][1])
    assert out[7]["pnp"][1] >= 40
    # below four pairs nothing is solved: the pose the frame starts the optimisation from is the copy of the frame before
    assert int(out[20]["status"]["n_landmarks"]) > 49 and int(out[20]["status"]["last_track_num"]) == 0


def test_depthless_landmarks_stay_out_of_the_pairs(P):
    st, out = oracle_run(P, "vo_depthless")
    n_with = st.notes["with_depth"]
    assert 20 <= n_with <= 29
    for k in (8, 9, 10, 11):
        assert out[k]["pnp"][1] == n_with, (k, out[k]["pnp"][1])      # 49 observations, only the landmarks with a depth are pairs
        assert len(st.frames()[k][1]) == 49
    assert out[7]["pnp"][1] == 49 and out[-1]["pnp"][1] == 49         # once triangulated from the returned depth pixels they are pairs again


def test_half_turn_start_rotation_passes_through_pi(P):
    st, out = oracle_run(P, "vo_half_turn")
    ang = np.array([np.degrees(np.linalg.norm(r["pnp"][2])) for r in out])
    rv = [r["pnp"][2] for r in out]
    flips = [k for k in range(st.cfg.window_size + 2, len(out)) if rv[k] @ rv[k - 1] < 0]
    assert len(flips) == 1, flips
    k = flips[0]
    assert 178.0 < ang[k - 1] <= 180.0 and 178.0 < ang[k] <= 180.0, (ang[k - 1], ang[k])     # within 2 degrees of pi on both sides
    assert ang[5] < 130 and ang[-1] < 130 and all(20 <= r["pnp"][1] for r in out[5:]) and all(30 <= len(f[1]) <= 48 for f in st.frames())
    # the oracle follows the turn (the world frame is the first body frame, which RingScene puts at the identity): attitude within a degree,
    # position within 0.1 m of the truth over the 224 degrees
    import excalib_ref as X
    for i, r in enumerate(out):
        if i < st.cfg.window_size:
            continue
        p, R = st.scene.pose(st.stamps[i])
        q = r["window"][-1, 3:7]
        assert X.rot_angle_deg(X.q2R(q), R) < 1.0 and np.abs(r["window"][-1, :3] - p).max() < 0.1, i


def test_standstill_starts_at_the_optimum_and_identity_extrinsic_at_zero(P):
    st, out = oracle_run(P, "vo_standstill")
    W = st.cfg.window_size
    for k in range(W + 7, len(out)):      # at rest: the start handed to solvePnP is the pose the window already holds
        assert np.abs(out[k]["pnp"][2] - out[k - 1]["pnp"][2]).max() < 1e-7 and np.abs(out[k]["pnp"][3] - out[k - 1]["pnp"][3]).max() < 1e-7, k
    st, out = oracle_run(P, "vo_identity_extrinsic")
    called, pairs, rv, tv = out[W + 1]["pnp"]
    assert called == 1 and pairs == 49 and not rv.any() and not tv.any()       # the first start vector is exactly zero: prev = 0 in the stop test
    assert all(not r["pnp"][2].any() for r in out[W + 1:])
