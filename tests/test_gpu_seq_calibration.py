"""Per-sequence calibration (vio_set_calibration): a slot with calibration k computes, bit for bit, what slot 0 of a one-sequence handle
created with the handle's configuration and k's fields computes, and matches the oracle run with that configuration.  Every sequence is
rendered once with the camera of its own calibration (vio_ct.synth_like(batch.config_of(i))) and the same frames and IMU go to every side."""
import os

import numpy as np
import pytest

import vio_ct

pytestmark = pytest.mark.gpu

SEQS = (3, 8, 13, 21)
N_RENDER = 44   # frames rendered per sequence (once per module)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def calibrations(P, cfg):
    """four rigs: the configuration's own, and three with other intrinsics, distortion, extrinsic, td / tr, IMU noise and gravity"""
    base = P.calibration_from_config(cfg)
    R0 = np.array(base.ric[:]).reshape(3, 3)
    out = [base]
    for fs, dc, dist, axis, deg, dt, noise, g, td, tr in (
            (1.05, (8, -6), False, (0, 0, 1), 3.0, (0.03, -0.02, 0.01), 0.5, 9.78, 0.02, 0.0),
            (0.95, (-8, 8), True, (1, 0, 0), -2.5, (-0.02, 0.03, 0.0), 4.0, 9.83, -0.02, 0.03),
            (1.02, (5, 8), True, (0, 1, 0), 2.0, (0.01, 0.01, -0.03), 2.0, 9.80, 0.0, 0.03)):
        k = P.Calibration()
        P._copy_fields(k, base)
        k.fx, k.fy = base.fx * fs, base.fy * (2.0 - fs)
        k.cx, k.cy = base.cx + dc[0], base.cy + dc[1]
        if not dist:
            k.k1 = k.k2 = k.p1 = k.p2 = 0.0
        R = _rot(axis, deg) @ R0
        for i in range(9):
            k.ric[i] = float(R.ravel()[i])
        for i in range(3):
            k.tic[i] = base.tic[i] + dt[i]
        k.acc_n, k.gyr_n, k.acc_w, k.gyr_w = base.acc_n * noise, base.gyr_n * noise, base.acc_w * noise, base.gyr_w * noise
        k.g_norm, k.td, k.tr = g, td, tr
        out.append(k)
    return out


FLAVOURS = {
    "default": (dict(), {}, 0),
    "free_ext_td": (dict(fix_depth=0, estimate_extrinsic=1, estimate_td=1), {}, 0),
    "dynamic_init": (dict(dynamic_init=1), {}, 0),
    "vo": (dict(use_imu=0, lk_max_level=3, estimate_td=0), {}, 0),
    "solve_mode_0": (dict(), {"VIO_SOLVE_MODE": "0"}, 0),
    "tracker_lag": (dict(), {}, 1),
    "ex_calib_2": (dict(estimate_extrinsic=2), {}, 0),
}

_frames = {}


def _scene(P, cfg, flavour, i, seq, n):
    """(synth config, frames, imu, td) of sequence seq with the camera of cfg (rendered once per module)"""
    sc = vio_ct.synth_like(cfg)
    if flavour == "vo":
        sc.t_static = 0.0
    key = (flavour == "vo", i, seq)
    syn = P.Synth(sc)
    if key not in _frames:
        _frames[key] = [syn.render_host(seq, float(t)) for t in vio_ct.frame_times(sc, N_RENDER)]
    assert n <= N_RENDER
    return sc, _frames[key][:n], syn.imu(seq, int(N_RENDER / sc.cam_rate * sc.imu_rate) + 64), cfg.td


def _snapshot(b, i):
    st = b.status(i)
    s = {k: getattr(st, k) for k, _ in type(st)._fields_}
    pr = b.prior(i)
    return dict(window=b.window(i), tracks=b.tracks(i), landmarks=b.landmarks(i), prior=pr, hist=b.odometry_history(i), status=s,
                extrinsic=b.extrinsic(i), latest=b.latest_odometry(i))


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    return a == b or (a != a and b != b)


class Env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _feed_all(handles, scenes, n, f0=0, f1=None, hook=None, t_off=0.0, kimu=None):
    """handles: [(batch, [(slot, scene index)])]; feeds frames f0..f1 of every scene to its slot(s), IMU pushed frame by frame"""
    f1 = n if f1 is None else f1
    kimu = kimu if kimu is not None else {}
    for f in range(f0, f1):
        for b, slots in handles:
            g = np.stack([scenes[j][1][f][0] for _, j in slots])
            d = np.stack([scenes[j][1][f][1] for _, j in slots])
            for s, j in slots:
                sc, _, (ti, ai, gi), td = scenes[j]
                tf = f / sc.cam_rate
                k = kimu.get((id(b), s), 0)
                k2 = vio_ct.imu_until(ti, k, tf + max(td, 0.0), sc.imu_rate)   # IMU through stamp + td (vio_feed's contract)
                if k2 > k:
                    b.push_imu(s, ti[k:k2] + t_off, ai[k:k2], gi[k:k2])
                kimu[(id(b), s)] = k2
            b.feed(g, d, [f / scenes[slots[0][1]][0].cam_rate + t_off] * len(slots))
        if hook is not None:
            hook(f)
    return kimu


def _setup(P, flavour, n, td_nonpos=False):
    kw, env, lag = FLAVOURS[flavour]
    cfg = P.canonical_config(**kw)
    cals = calibrations(P, cfg)
    if td_nonpos:   # vio_ct's oracle driver pushes IMU only through the frame stamp: a positive td would starve its IMU wait
        for k in cals:
            k.td = -abs(k.td)
    with Env(env):
        b = P.VioBatch(cfg, len(cals))
        for i, k in enumerate(cals):
            b.set_calibration(i, k)
        singles = [P.VioBatch(b.config_of(i), 1) for i in range(len(cals))]
    if lag:
        b.set_tracker_lag(lag)
        for h in singles:
            h.set_tracker_lag(lag)
    scenes = [_scene(P, b.config_of(i), flavour, i, SEQS[i], n) for i in range(len(cals))]
    return cfg, cals, b, singles, scenes


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_heterogeneous_batch_equals_single_handles(P, flavour):
    n = 30
    cfg, cals, b, singles, scenes = _setup(P, flavour, n)
    handles = [(b, [(i, i) for i in range(len(cals))])] + [(h, [(0, i)]) for i, h in enumerate(singles)]
    inits = [0] * len(cals)

    def check(f):
        for i, h in enumerate(singles):
            a, z = _snapshot(b, i), _snapshot(h, 0)
            for k in a:
                assert _same(a[k], z[k]), (flavour, i, f, k)
            inits[i] = max(inits[i], a["status"]["solver_flag"])

    _feed_all(handles, scenes, n, hook=check)
    if flavour == "ex_calib_2":                      # every slot ran the calibration phase (state 2 calibrating / 1 calibrated)
        assert all(b.ex_calibration(i)["state"] in (1, 2) and b.ex_calibration(i)["pairs"] > 0 for i in range(len(cals)))
    elif flavour in ("vo", "dynamic_init"):
        assert max(inits) == 1, inits                # at least one rig initialised on these slower starts
    else:
        assert all(x == 1 for x in inits), inits     # every rig initialised and tracks


def test_each_sequence_matches_the_oracle_with_its_calibration(P):
    n = 34
    cfg, cals, b, singles, scenes = _setup(P, "free_ext_td", n, td_nonpos=True)
    stat = [[] for _ in cals]
    traj = [[] for _ in cals]

    def rec(f):
        for i in range(len(cals)):
            st = b.status(i)
            stat[i].append((st.solver_flag, st.frame_count, st.n_landmarks, st.processed, st.marginalization_flag))
            if st.solver_flag == 1 and st.processed:
                w = b.window(i)
                traj[i].append((f, w[cfg.window_size, :3].copy(), w[cfg.window_size, 3:7].copy()))

    _feed_all([(b, [(i, i) for i in range(len(cals))])], scenes, n, hook=rec)
    for i in range(len(cals)):
        ci = b.config_of(i)
        o = vio_ct.run_oracle_sequence(ci, scenes[i][0], SEQS[i], n, frames=scenes[i][1])
        for f in range(n):
            so, sh = o["status"][f], stat[i][f]
            assert (int(so["solver_flag"]), int(so["frame_count"]), int(so["n_landmarks"])) == sh[:3], (i, f)
            if sh[0] == 1 and sh[3]:
                assert int(so["marginalization_flag"]) == sh[4], (i, f)
        assert len(traj[i]) == len(o["traj"]) > 10
        po = np.array([x[1] for x in o["traj"]]); ph = np.array([x[1] for x in traj[i]])
        qo = np.array([x[2] for x in o["traj"]]); qh = np.array([x[2] for x in traj[i]])
        assert np.abs(po - ph).max() < 1e-5, (i, float(np.abs(po - ph).max()))
        assert np.abs(np.abs((qo * qh).sum(1)) - 1).max() < 1e-9
        gt = np.array(o["gt"])
        ate_o, ate_h = vio_ct.ate_rmse(po, gt), vio_ct.ate_rmse(ph, gt)
        # the renderer has no time offset: a slot configured with td = -20 ms starts from a calibration error it has to work off
        bar = 0.03 if cals[i].td == 0 else 0.05
        assert ate_o < bar and ate_h < bar, (i, ate_o, ate_h)
        assert abs(ate_h - ate_o) <= max(0.01 * ate_o, 2e-4)
        a, q = o["oracle"].tracks(), b.tracks(i)
        assert np.array_equal(a[0], q[0]) and np.array_equal(a[1], q[1])


def test_calibration_change_mid_run_restarts_only_that_slot(P):
    n, c0 = 44, 18
    cfg, cals, b, singles, scenes = _setup(P, "default", n)
    ref = P.VioBatch(cfg, len(cals))     # the batch without the change
    for i, k in enumerate(cals):
        ref.set_calibration(i, k)
    new_cal = cals[2]
    fresh = P.VioBatch(P.config_with_calibration(cfg, new_cal), 1)   # rig 2 on a new handle, fed from stamp 0
    alt = scenes[2]                        # rig 2's camera and recording (config_of(2) is that configuration)
    both = [(b, [(i, i) for i in range(4)]), (ref, [(i, i) for i in range(4)])]
    ki = _feed_all(both, scenes, n, 0, c0)
    assert b.status(1).solver_flag == 1
    b.set_calibration(1, new_cal)          # slot 1 now serves rig 2, whose clock starts again at 0
    assert b.status(1).solver_flag == 0 and b.status(1).frame_count == 0
    ki[(id(b), 1)] = 0
    for f in range(n - c0):
        g, d, stamps = [], [], []
        for s in range(4):
            sc, fr, (ti, ai, gi), td = alt if s == 1 else scenes[s]
            ff = f if s == 1 else c0 + f
            tf = ff / sc.cam_rate
            k = ki.get((id(b), s), 0)
            k2 = vio_ct.imu_until(ti, k, tf + max(td, 0.0), sc.imu_rate)
            if k2 > k:
                b.push_imu(s, ti[k:k2], ai[k:k2], gi[k:k2])
            ki[(id(b), s)] = k2
            g.append(fr[ff][0]); d.append(fr[ff][1]); stamps.append(tf)
        b.feed(np.stack(g), np.stack(d), stamps)
        _feed_all([(fresh, [(0, 0)])], [alt], n, f, f + 1, kimu=ki)
        _feed_all([(ref, [(i, i) for i in range(4)])], scenes, n, c0 + f, c0 + f + 1, kimu=ki)
        a, z = _snapshot(b, 1), _snapshot(fresh, 0)
        for k in a:
            assert _same(a[k], z[k]), (f, k)
        for s in (0, 2, 3):
            a, z = _snapshot(b, s), _snapshot(ref, s)
            for k in a:
                assert _same(a[k], z[k]), (s, f, k)
    assert fresh.status(0).solver_flag == 1


def test_calibration_survives_resets_and_reboot(P):
    n = 44
    cfg, cals, b, singles, scenes = _setup(P, "default", n)
    # the failure-detection recipe of test_gpu_edge: blank frames and a violent accelerometer offset on slot 2
    sc, frames, (ti, ai, gi), td = scenes[2]
    frames = list(frames)
    blank = (np.full_like(frames[0][0], 90), frames[0][1])
    for f in (18, 19, 20, 21, 22):
        frames[f] = blank
    ai = ai.copy()
    ai[(ti > 1.8) & (ti < 2.3), 0] += 80.0
    scenes[2] = (sc, frames, (ti, ai, gi), td)
    handles = [(b, [(i, i) for i in range(4)])] + [(h, [(0, i)]) for i, h in enumerate(singles)]
    reboots = []

    def check(f):
        if f == 12:
            b.reset_seq(3); singles[3].reset_seq(0)
        if f == 16:
            b.reset_tracker_seq(1); singles[1].reset_tracker_seq(0)
        for i, h in enumerate(singles):
            a, z = _snapshot(b, i), _snapshot(h, 0)
            for k in a:
                assert _same(a[k], z[k]), (i, f, k)
        if b.status(2).code == P.VIO_REBOOTED:
            reboots.append(f)
            e = b.extrinsic(2)
            k = b.calibration(2)
            assert np.array_equal(e[3:12], np.array(k.ric[:])) and np.array_equal(e[0:3], np.array(k.tic[:]))
            assert not np.array_equal(e[3:12], np.array(cfg.ric[:]))
            assert e[12] == k.td

    _feed_all(handles, scenes, n, hook=check)
    assert reboots, "the reboot recipe did not fire"
    # vio_reset keeps every slot's calibration
    b.reset()
    for i, k in enumerate(cals):
        got = b.calibration(i)
        assert got.fx == k.fx and got.g_norm == k.g_norm and got.acc_n == k.acc_n
        e = b.extrinsic(i)
        assert np.array_equal(e[3:12], np.array(got.ric[:]))


def test_round_trip_and_refusals(P):
    cfg = P.canonical_config()
    cals = calibrations(P, cfg)
    b = P.VioBatch(cfg, 3)
    k = cals[2]
    b.set_calibration(1, k)
    got = b.calibration(1)
    for f in P.CALIBRATION_FIELDS:
        if f != "ric":
            assert np.array_equal(np.array(getattr(got, f), ndmin=1), np.array(getattr(k, f), ndmin=1)), f
    R = np.array(got.ric[:]).reshape(3, 3)
    # (the configuration's ric is orthonormal to ~1e-8 only: re-orthonormalisation moves it by that much)
    assert np.abs(R - np.array(k.ric[:]).reshape(3, 3)).max() < 1e-7 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    # the slot at creation holds the configuration's calibration (ric re-orthonormalised like cfg.ric)
    e = b.extrinsic(0)
    assert np.array_equal(e[3:12], np.array(b.calibration(0).ric[:]))
    before = [_snapshot(b, s) for s in range(3)]
    cal_before = [bytes(b.calibration(s)) for s in range(3)]
    bad = []
    for field, val in (("fx", 0.0), ("fy", -1.0), ("cx", float("nan")), ("k1", float("inf")), ("tr", -0.01), ("acc_n", 0.0),
                       ("acc_w", -1e-3), ("gyr_n", 0.0), ("gyr_w", float("nan")), ("g_norm", 0.0), ("td", float("nan"))):
        x = P.Calibration(); P._copy_fields(x, k); setattr(x, field, val); bad.append((field, x))
    for field, R in (("ric", np.diag([1.0, 1.0, 1.0 + 1e-5])), ("ric", np.diag([1.0, 1.0, -1.0]))):
        x = P.Calibration(); P._copy_fields(x, k)
        for i in range(9):
            x.ric[i] = float(R.ravel()[i])
        bad.append((field, x))
    x = P.Calibration(); P._copy_fields(x, k); x.tic[1] = float("inf"); bad.append(("tic", x))
    for field, x in bad:
        with pytest.raises(P.VioError) as ei:
            b.set_calibration(2, x)
        assert field in str(ei.value), (field, str(ei.value))
    for seq in (-1, 3):
        with pytest.raises(P.VioError):
            b.set_calibration(seq, k)
        assert b.L.vio_get_calibration(b.h, seq, None) == P.VIO_EINVAL
    assert [bytes(b.calibration(s)) for s in range(3)] == cal_before
    after = [_snapshot(b, s) for s in range(3)]
    assert _same(before, after)
    # mode 2: the slot's extrinsic is I / 0 whatever was set
    b2 = P.VioBatch(P.canonical_config(estimate_extrinsic=2), 2)
    b2.set_calibration(1, k)
    g2 = b2.calibration(1)
    assert np.array_equal(np.array(g2.ric[:]), np.eye(3).ravel()) and np.array_equal(np.array(g2.tic[:]), np.zeros(3))
    assert g2.fx == k.fx and g2.acc_n == k.acc_n


def test_replay_many_writes_what_each_recording_writes_alone(P, tmp_path):
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    cfg = P.canonical_config()
    cals = calibrations(P, cfg)[1:4]
    for k in cals:
        k.td = -abs(k.td)   # replay() pushes IMU one sample beyond the frame stamp
    lens = (22, 28, 25)
    yamls, recs, dirs = [], [], []
    for j, (k, n) in enumerate(zip(cals, lens)):
        c = P.config_with_calibration(cfg, k)
        sc = vio_ct.synth_like(c)
        syn = P.Synth(sc)
        t = vio_ct.frame_times(sc, n)
        frames = _frames.get((False, j + 1, SEQS[j + 1]))   # the default flavour's scene of this rig, if rendered already
        frames = frames[:n] if frames is not None else [syn.render_host(SEQS[j + 1], float(x)) for x in t]
        ti, ai, gi = syn.imu(SEQS[j + 1], int(n / sc.cam_rate * sc.imu_rate) + 64)
        d = str(tmp_path / ("rec%d" % j))
        io.write_recording(d, t, [f[0] for f in frames], [f[1] for f in frames], ti, ai, gi)
        R = np.array(k.ric[:]).reshape(3, 3)
        y = tmp_path / ("cam%d.yaml" % j)
        y.write_text("%%YAML:1.0\nimage_width: %d\nimage_height: %d\nmax_cnt: %d\nmin_dist: %d\nnum_grid_rows: %d\nnum_grid_cols: %d\n"
                     "fix_depth: %d\ndepth_min_dist: %r\ndepth_max_dist: %r\nF_threshold: %r\nmax_num_iterations: %d\nkeyframe_parallax: %r\n"
                     "acc_n: %r\nacc_w: %r\ngyr_n: %r\ngyr_w: %r\ng_norm: %r\nestimate_extrinsic: 0\nestimate_td: 0\ntd: %r\n"
                     "rolling_shutter: %d\nrolling_shutter_tr: %r\n"
                     "projection_parameters:\n   fx: %r\n   fy: %r\n   cx: %r\n   cy: %r\n"
                     "distortion_parameters:\n   k1: %r\n   k2: %r\n   p1: %r\n   p2: %r\n"
                     "extrinsicRotation: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [%s]\n"
                     "extrinsicTranslation: !!opencv-matrix\n   rows: 3\n   cols: 1\n   dt: d\n   data: [%s]\n"
                     % (cfg.width, cfg.height, cfg.max_cnt, cfg.min_dist, cfg.grid_rows, cfg.grid_cols, cfg.fix_depth, cfg.depth_min,
                        cfg.depth_max, cfg.f_threshold, cfg.max_iterations, cfg.min_parallax_px, k.acc_n, k.acc_w, k.gyr_n, k.gyr_w,
                        k.g_norm, k.td, 1 if k.tr > 0 else 0, k.tr, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2,
                        ", ".join(repr(float(v)) for v in R.ravel()), ", ".join(repr(float(v)) for v in k.tic)))
        yamls.append(str(y)); dirs.append(d)
        recs.append(io.RgbdImuDirectory(d))
    shared, kk, extras = io.batch_config_from_yamls(yamls, P)
    b = P.VioBatch(shared, 3, imu_capacity=1 << 15)
    for i, k in enumerate(kk):
        b.set_calibration(i, k)
    outs = [str(tmp_path / ("many%d.csv" % i)) for i in range(3)]
    rows = io.replay_many(b, recs, outs)
    for i in range(3):
        c, e = io.config_from_yaml(yamls[i], P)
        one = P.VioBatch(c, 1, imu_capacity=1 << 15)
        alone = str(tmp_path / ("alone%d.csv" % i))
        r1 = io.replay(one, recs[i], alone)
        assert len(r1) > 5 and np.array_equal(r1, rows[i]), i
        assert open(alone).read() == open(outs[i]).read(), i
