"""estimate_extrinsic = 2 on the GPU: the device solveRelativeR (vio_stage_relative_r) and the calibration phase of be_ingest<true> against
the numpy restatement of InitialEXRotation (tests/excalib_ref.py), driven through vio_process_obs by the test-side three-axis generator."""

import numpy as np
import pytest

import excalib_ref as X
import vio_ct

pytestmark = pytest.mark.gpu


def _relative_r_case(rs, n, noise_px, R, t):
    Xl = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(3, 9, n)], 1)
    Xr = (Xl - t) @ R
    xl, xr = Xl / Xl[:, 2:], Xr / Xr[:, 2:]
    xl[:, :2] += rs.normal(0, noise_px / 460.0, (n, 2))
    xr[:, :2] += rs.normal(0, noise_px / 460.0, (n, 2))
    return np.ascontiguousarray(np.hstack([xl, xr]))


def _device_relative_r(P, co):
    out = np.zeros(9)
    assert P.lib().vio_stage_relative_r(len(co), co.ctypes.data, out.ctypes.data) == 0
    return out.reshape(3, 3)


def test_stage_relative_r_matches_restatement(P):
    """9, 14, 15, 150, 300 correspondences, 0 and 0.5 px noise, several motions: the same R1 / R2 choice everywhere and the same matrix to 1e-9
    where the 8-point system is well-conditioned (noise-free, >= 15 points; 1e-6 otherwise); both R1 and R2 win somewhere"""
    rs = np.random.RandomState(11)
    wins = set()
    for n in (9, 14, 15, 150, 300):
        for noise in (0.0, 0.5):
            for m in range(4):
                R = X.rodrigues(rs.normal(0, 0.15, 3))
                t = rs.normal(0, 0.3, 3)
                co = _relative_r_case(rs, n, noise, R, t)
                ref, d = X.solve_relative_r(co, detail=True)
                dev = _device_relative_r(P, co)
                wins.add(d["win"])
                other = d["R2"] if d["win"] == 1 else d["R1"]
                assert np.abs(dev - ref).max() < np.abs(dev - other).max(), (n, noise, m)   # the same choice
                tol = 1e-9 if (noise == 0.0 and n >= 15) else 1e-6
                assert np.abs(dev - ref).max() < tol, (n, noise, m, np.abs(dev - ref).max())
                if noise == 0.0:
                    assert X.rot_angle_deg(dev, R) < 1e-3
    assert wins == {1, 2}, wins
    # pure rotation: E is undetermined; the result is still a proper rotation, and fewer than 9 points give the identity
    co = _relative_r_case(rs, 100, 0.5, X.rodrigues([0.05, 0.1, -0.02]), np.zeros(3))
    dev = _device_relative_r(P, co)
    assert abs(np.linalg.det(dev) - 1) < 1e-9 and np.abs(dev @ dev.T - np.eye(3)).max() < 1e-9
    assert np.array_equal(_device_relative_r(P, co[:8].copy()), np.eye(3))


class Driver:
    """feeds S generator scenes through vio_process_obs, one frame per call of step()"""

    def __init__(self, P, cfg, scenes, n_frames):
        self.b = P.VioBatch(cfg, len(scenes))
        self.scenes = scenes
        self.imu = [sc.imu(sc.frame_time(n_frames) + 0.5) for sc in scenes]
        self.k_imu = [0] * len(scenes)
        self.k = 0

    def step(self):
        for s, sc in enumerate(self.scenes):
            t = sc.frame_time(self.k)
            ts, acc, gyr = self.imu[s]
            k2 = X.imu_until(ts, self.k_imu[s], t)
            if k2 > self.k_imu[s]:
                self.b.push_imu(s, ts[self.k_imu[s]:k2], acc[self.k_imu[s]:k2], gyr[self.k_imu[s]:k2])
            self.k_imu[s] = k2
            ids, obs, depth = sc.frame(t)
            self.b.process_obs(s, ids, obs, depth, t)
        self.k += 1


def _check_against_restatement(e, W):
    """the device's estimate and singular values against the restatement applied to the device's own history"""
    ric, sv, ok, lam = X.average(e["history"], e["pairs"], W)
    assert np.abs(e["sv"][:3] - sv[:3]).max() < 1e-10, (e["sv"], sv)
    assert abs(e["sv"][3] ** 2 - lam[3]) < 1e-10
    if sv[2] > 1e-3:   # the smallest eigenvector is defined
        assert np.abs(e["ric"] - ric).max() < 1e-10, np.abs(e["ric"] - ric).max()
    return ok


def test_averaging_matches_restatement_frame_by_frame(P):
    """S = 8 phases: every frame, every sequence, until its calibration succeeds; the success frame is the restatement's first success"""
    cfg = P.canonical_config(estimate_extrinsic=2)
    W = cfg.window_size
    d = Driver(P, cfg, [X.Scene(cfg, phase=0.4 * s) for s in range(8)], 40)
    done = [False] * 8
    for f in range(40):
        d.step()
        for s in range(8):
            if done[s]:
                continue
            e = d.b.ex_calibration(s, history=True)
            assert e["pairs"] == f, (s, f, e["pairs"])
            if f == 0:
                continue
            ok = _check_against_restatement(e, W)
            assert (e["state"] == 1) == ok, (s, f, e["state"], ok)
            if ok:
                assert e["success_frame"] == f + 1 == d.b.status(s).frames_processed
                done[s] = True
    assert all(done), done


def _ate_yaw_aligned(est, true):
    est, true = np.asarray(est), np.asarray(true)
    ce, ct = est.mean(0), true.mean(0)
    a, b = est - ce, true - ct
    th = np.arctan2((a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum(), (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).sum())
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    return float(np.sqrt((((a @ Rz.T) - b) ** 2).sum(1).mean()))


def test_convergence_and_refinement(P):
    """Noise-free: the device succeeds at the call the CPU restatement predicts (excalib_ref.predict_success), within 0.1 deg of ric_true.
    Then 150 more frames: the ATE after yaw alignment stays within 1.5x that of a mode-1 run given ric_true / tic_true, and the refined tic
    ends closer to tic_true than the zero it starts from.
    Measured on an MI355X: success at frames_processed 21 (call 20, as predicted), 0.0052 deg from ric_true, singular values 0.759 0.725
    0.263 8.1e-5.  After 150 more frames: mode 2 ATE 0.76 m (one failure-detection reboot), mode 1 2.38 m (two reboots) -- this trajectory
    (1.5 rad/s about all three axes) is harsh for the estimator in both modes, so the ATE bound is a weak check; refined tic 4.5 mm from
    tic_true (mode 1: 3.6 mm), ric 0.010 deg from ric_true."""
    cfg = P.canonical_config(estimate_extrinsic=2)
    sc = X.Scene(cfg, phase=0.0)
    k_pred, _ = X.predict_success(sc)
    n = k_pred + 1 + 150
    runs = {}
    for mode in (2, 1):
        c = cfg
        if mode == 1:
            c = P.canonical_config(estimate_extrinsic=1)
            for i in range(9):
                c.ric[i] = float(X.RIC_TRUE.ravel()[i])
            for i in range(3):
                c.tic[i] = float(X.TIC_TRUE[i])
        d = Driver(P, c, [X.Scene(c, phase=0.0)], n)
        est, true = [], []
        for f in range(n):
            d.step()
            st = d.b.status(0)
            if mode == 2 and f == k_pred:
                e = d.b.ex_calibration(0)
                assert e["state"] == 1 and e["success_frame"] == k_pred + 1, (e["state"], e["success_frame"], k_pred)
                ang = X.rot_angle_deg(e["ric"], X.RIC_TRUE)
                assert ang < 0.1, ang
            if st.solver_flag == 1:
                w = d.b.window(0)
                est.append(w[-1, :3])
                true.append(sc.pose(w[-1, 16])[0])
        assert len(est) > 100, len(est)
        runs[mode] = (_ate_yaw_aligned(est, true), d.b.extrinsic(0))
    ate2, ate1 = runs[2][0], runs[1][0]
    assert ate2 <= 1.5 * max(ate1, 1e-3), (ate2, ate1)
    tic = runs[2][1][:3]
    assert np.linalg.norm(tic - X.TIC_TRUE) < np.linalg.norm(X.TIC_TRUE), tic


@pytest.mark.parametrize("dyn", [0, 1])
def test_initialisation_gate_per_sequence(P, dyn):
    """a mixed batch: pure translations never calibrate and stay INITIAL (frame_count saturates at W, frames keep counting, no solve runs),
    the rotating sequences calibrate, and with the static initialisation they initialise"""
    cfg = P.canonical_config(estimate_extrinsic=2, dynamic_init=dyn)
    W = cfg.window_size
    scenes = [X.Scene(cfg, phase=0.0), X.Scene(cfg, rot=0.0, phase=1.0), X.Scene(cfg, phase=2.0), X.Scene(cfg, rot=0.0, phase=3.0)]
    d = Driver(P, cfg, scenes, 40)
    for f in range(40):
        d.step()
        for s in (1, 3):
            st, e = d.b.status(s), d.b.ex_calibration(s)
            assert e["state"] == 2 and st.solver_flag == 0 and st.frame_count == min(f + 1, W) and st.frames_processed == f + 1
            assert st.solves_total == 0 and st.overflow_flags == 0
        for s in (0, 2):
            st, e = d.b.status(s), d.b.ex_calibration(s)
            if e["state"] == 2:
                assert st.solver_flag == 0 and st.solves_total == 0
    for s in (0, 2):
        assert d.b.ex_calibration(s)["state"] == 1
        if not dyn:
            assert d.b.status(s).solver_flag == 1


def test_reset_semantics(P):
    """vio_reset_seq keeps the calibrated rotation with tic = 0 and stays calibrated; vio_reset starts over; mode 2 without IMU is refused"""
    cfg = P.canonical_config(estimate_extrinsic=2)
    d = Driver(P, cfg, [X.Scene(cfg, phase=0.0)], 30)
    for f in range(30):
        d.step()
    e = d.b.ex_calibration(0)
    assert e["state"] == 1
    d.b.reset_seq(0)
    e2 = d.b.ex_calibration(0)
    assert e2["state"] == 1 and np.array_equal(e2["ric"], e["ric"]) and e2["success_frame"] == e["success_frame"]
    ex = d.b.extrinsic(0)
    assert np.array_equal(ex[3:12].reshape(3, 3), e["ric"]) and np.array_equal(ex[:3], np.zeros(3))
    d.b.reset()
    e3 = d.b.ex_calibration(0)
    assert e3["state"] == 2 and e3["pairs"] == 0 and e3["success_frame"] == -1 and np.array_equal(e3["ric"], np.eye(3))
    assert np.array_equal(d.b.extrinsic(0)[3:12].reshape(3, 3), np.eye(3))
    with pytest.raises(Exception):
        P.VioBatch(P.canonical_config(estimate_extrinsic=2, use_imu=0), 1)


def test_feed_path_mode2(P):
    """vio_feed on the synthetic renderer, 60 frames, canonical_config: no capacity flag, one pair per processed frame after the first, the
    sequences stay INITIAL (the motion is too gentle to calibrate), and the averaging still matches the restatement"""
    cfg = P.canonical_config(estimate_extrinsic=2)
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    S, n_frames = 2, 60
    b = P.VioBatch(cfg, S)
    imu = [syn.imu(s, int(n_frames / sc.cam_rate * sc.imu_rate) + 64) for s in range(S)]
    k = [0] * S
    for f, tf in enumerate(vio_ct.frame_times(sc, n_frames)):
        for s in range(S):
            ti, ai, gi = imu[s]
            k2 = vio_ct.imu_until(ti, k[s], tf, sc.imu_rate)
            if k2 > k[s]:
                b.push_imu(s, ti[k[s]:k2], ai[k[s]:k2], gi[k[s]:k2])
            k[s] = k2
        fr = [syn.render_host(s, tf) for s in range(S)]
        b.feed(np.stack([g for g, _ in fr]), np.stack([dd for _, dd in fr]), [tf] * S)
        for s in range(S):
            st = b.status(s)
            assert st.overflow_flags == 0 and st.solver_flag == 0
            e = b.ex_calibration(s, history=True)
            assert e["state"] == 2 and e["pairs"] == max(st.frames_processed - 1, 0)
            if e["pairs"] > 0:
                _check_against_restatement(e, cfg.window_size)
    assert all(b.status(s).frames_processed > 40 for s in range(S))


def test_full_calibration_history_raises_flag_128_and_keeps_the_latest_pairs(P):
    """A rotation about one axis never calibrates (tests/test_ex_calib_cpu.py): every frame adds a pair until the ring of VIO_EXCALIB_CAP =
    2048 pairs is full.  From the first dropped pair on every frame carries overflow flag 128 and code VIO_ECAPACITY -- flag 128 means only
    "calibration history full" (ABI 8; the fallback solver's deviation is flag 512, which never appears here) -- and the history holds the
    latest 2048 pairs, oldest first."""
    cap, extra = 2048, 4
    cfg = P.canonical_config(estimate_extrinsic=2)
    sc = X.Scene(cfg, phase=0.0, axes=(1.0, 0.0, 0.0))
    assert X.predict_success(sc, max_frames=60)[0] is None
    n = cap + 1 + extra                   # the frame of index f >= 1 adds pair f: index cap + 1 drops the first
    d = Driver(P, cfg, [sc], n)
    full = None
    for f in range(n):
        d.step()
        st, e = d.b.status(0), d.b.ex_calibration(0)
        assert e["state"] == 2 and st.solver_flag == 0, (f, e["state"])
        assert st.overflow_flags & 512 == 0, (f, st.overflow_flags)
        if f <= cap:
            assert e["pairs"] == f and st.overflow_flags == 0 and st.code == P.VIO_OK, (f, e["pairs"], st.overflow_flags, st.code)
        else:
            assert e["pairs"] == cap and st.overflow_flags == 128 and st.code == P.VIO_ECAPACITY, (f, e["pairs"], st.overflow_flags, st.code)
        if f == cap:
            full = d.b.ex_calibration(0, history=True)
    dropped = n - 1 - cap
    assert st.overflow_frames == dropped, st.overflow_frames
    e = d.b.ex_calibration(0, history=True)
    assert e["history"].shape == (cap, 3, 4)
    assert np.array_equal(e["history"][:cap - dropped], full["history"][dropped:])   # the oldest went first
    # the newest pairs sit at the end, in frame order: their IMU rotation is the relative body rotation of their two frames
    for j in range(dropped + 1):
        _, Rl = sc.pose(sc.frame_time(n - 2 - j))
        _, Rr = sc.pose(sc.frame_time(n - 1 - j))
        assert X.rot_angle_deg(X.q2R(e["history"][cap - 1 - j][1]), Rl.T @ Rr) < 0.05, j   # (neighbouring pairs differ by > 0.3 degrees)
    assert not X.average(e["history"], e["pairs"], cfg.window_size)[2] and e["sv"][2] < 0.25, e["sv"]
