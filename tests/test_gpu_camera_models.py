"""KANNALA_BRANDT and MEI camera models on the device: the device stage against the host stage, the device renderer against
the host renderer, vio_set_camera's refusals, MEI with xi = 0 against PINHOLE through the whole pipeline, per-slot cameras in one batch
against one-sequence handles, the published normalised points, the pose graph's keypoint lift, and trajectory accuracy per lens."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as cr  # noqa: E402
import vio_ct  # noqa: E402

pytestmark = pytest.mark.gpu


def _lenses(P):
    kb = P.camera_kannala_brandt(*(cr.KB_LENS[n] for n in P.CAMERA_PARAMS[P.CAMERA_KANNALA_BRANDT]))
    mei = P.camera_mei(*(cr.MEI_LENS[n] for n in P.CAMERA_PARAMS[P.CAMERA_MEI]))
    kb2 = P.camera_kannala_brandt(-0.02, 0.004, -0.0005, 0.0, 360.0, 355.0, 318.0, 242.0)
    return kb, mei, kb2


def _points():
    return np.concatenate([cr.grid(), cr.random_points(1500, 11)])


def test_device_stage_equals_host_stage(P):
    kb, mei, kb2 = _lenses(P)
    pin = P.camera_pinhole(P.canonical_config())
    a = 0.04
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    edge = [P.camera_kannala_brandt(*(k + (330.0, 330.0, 321.26, 239.71))) for k in cr.KB_EDGE.values()]
    for cam in [pin, kb, mei, kb2] + edge:
        uv = _points()
        rd, ud, od = P.stage_camera(cam, uv, R)
        rh, uh, oh = P.stage_host_camera(cam, uv, R)
        assert np.array_equal(rd, rh) and np.array_equal(ud, uh), cam          # the lift: + - * / sqrt and sincos_det only
        assert np.abs(od - oh).max() <= 1e-9, (cam, float(np.abs(od - oh).max()))   # atan2 of two math libraries


def test_device_and_host_renderers_agree(P):
    kb, mei, _ = _lenses(P)
    sc = P.default_synth()
    syn = P.Synth(sc)
    S, hw = 4, sc.width * sc.height
    g = P.DeviceBuffer(S * hw)
    d = P.DeviceBuffer(S * hw * 2)
    for cam in (kb, mei):
        for f in range(20):
            t = 1.0 + 0.1 * f
            syn.render_device(S, 40, t, g.at(0), d.at(0), camera=cam)
            gd = g.download(0, (S, sc.height, sc.width), np.uint8)
            dd = d.download(0, (S, sc.height, sc.width), np.uint16)
            for s in range(S):
                gh, dh = syn.render_host(40 + s, t, camera=cam)
                assert np.array_equal(gd[s], gh) and np.array_equal(dd[s], dh), (cam, f, s)
    g.free()
    d.free()


def test_set_camera_refusals_leave_slots_untouched(P):
    cfg = P.canonical_config()
    b = P.VioBatch(cfg, 3)
    kb, mei, _ = _lenses(P)
    b.set_camera(1, kb)
    before = [b.camera(i) for i in range(3)]
    cal_before = [b.calibration(i) for i in range(3)]

    def bad(base, idx, value, field):
        c = P.Camera()
        c.model, c.reserved = base.model, base.reserved
        for i in range(12):
            c.p[i] = base.p[i]
        if idx == "model":
            c.model = value
        elif idx == "reserved":
            c.reserved = value
        else:
            c.p[idx] = value
        with pytest.raises(P.VioError) as e:
            b.set_camera(1, c)
        assert "(-1)" in str(e.value) and field in str(e.value), (field, str(e.value))

    bad(kb, "model", 3, "model")
    bad(kb, "reserved", 1, "reserved")
    bad(kb, 0, float("nan"), "k2")
    bad(kb, 4, 0.0, "mu")
    bad(kb, 5, -1.0, "mv")
    bad(kb, 6, float("inf"), "u0")
    bad(mei, 0, -0.1, "xi")
    bad(mei, 5, 0.0, "gamma1")
    bad(mei, 6, -5.0, "gamma2")
    bad(mei, 1, float("nan"), "k1")
    pin = P.camera_pinhole(cfg)
    bad(pin, 0, 0.0, "fx")
    bad(pin, 1, -1.0, "fy")
    bad(pin, 7, float("nan"), "p2")
    bad(kb, 11, float("nan"), "p[11]")
    # a field of view reaching 90 degrees: KANNALA_BRANDT with mu = 100 puts the corners beyond pi / 2
    bad(kb, 4, 100.0, "pixel")
    bad(mei, 5, 150.0, "pixel")
    for i in range(3):
        assert b.camera(i) == before[i]
        assert bytes(b.calibration(i)) == bytes(cal_before[i])
    b.close()


def _feed(b, syn, seqs, frames_of, n, hook=None):
    """feeds slot i sequence seqs[i]'s IMU and frames_of(i, f, t)"""
    sc = syn.cfg
    S = len(seqs)
    imu = [syn.imu(s, int(n / sc.cam_rate * sc.imu_rate) + 64) for s in seqs]
    k = [0] * S
    for f, tf in enumerate(vio_ct.frame_times(sc, n)):
        for i in range(S):
            ti, ai, gi = imu[i]
            k2 = vio_ct.imu_until(ti, k[i], tf, sc.imu_rate)
            if k2 > k[i]:
                b.push_imu(i, ti[k[i]:k2], ai[k[i]:k2], gi[k[i]:k2])
            k[i] = k2
        fr = [frames_of(i, f, float(tf)) for i in range(S)]
        b.feed(np.stack([x[0] for x in fr]), np.stack([x[1] for x in fr]), [tf] * S)
        if hook is not None:
            hook(f, b)


def _same_state(a, i, b, j, what):
    assert np.array_equal(a.window(i), b.window(j)), what
    assert np.array_equal(a.landmarks(i), b.landmarks(j)), what
    ta, tb = a.tracks(i), b.tracks(j)
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(ta, tb)), what


def test_mei_xi_zero_slot_equals_pinhole_slot(P):
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    b = P.VioBatch(cfg, 2)
    b.set_camera(1, P.camera_mei(0.0, cfg.k1, cfg.k2, cfg.p1, cfg.p2, cfg.fx, cfg.fy, cfg.cx, cfg.cy))
    cache = {}

    def frames(i, f, t):
        if f not in cache:
            cache[f] = syn.render_host(7, t)
        return cache[f]

    def check(f, bb):
        _same_state(bb, 0, bb, 1, f)
        ia, oa = bb.packaged(0)
        ib, ob = bb.packaged(1)
        assert np.array_equal(ia, ib) and np.array_equal(oa, ob), f

    _feed(b, syn, [7, 7], frames, 60, hook=check)
    assert b.status(1).solver_flag == 1
    b.close()


def test_batch_of_cameras_equals_single_handles(P):
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    kb, mei, kb2 = _lenses(P)
    cams = [P.camera_pinhole(cfg), kb, mei, kb2]
    seqs = [21, 22, 23, 24]
    n = 40
    renders = {}

    def frames(i, f, t, off=0):
        key = (i + off, f)
        if key not in renders:
            renders[key] = syn.render_host(seqs[i + off], t, camera=cams[i + off])
        return renders[key]

    b = P.VioBatch(cfg, 4)
    for i in (1, 2, 3):
        b.set_camera(i, cams[i])
    snaps = []
    _feed(b, syn, seqs, frames, n, hook=lambda f, bb: snaps.append([(bb.window(i), bb.packaged(i)) for i in range(4)]))
    for i in range(4):
        a = P.VioBatch(cfg, 1)
        if i:
            a.set_camera(0, cams[i])
        k = []
        _feed(a, syn, [seqs[i]], lambda _i, f, t, i=i: frames(0, f, t, off=i), n, hook=lambda f, aa: k.append((aa.window(0), aa.packaged(0))))
        for f in range(n):
            assert np.array_equal(k[f][0], snaps[f][i][0]), (i, f)
            assert np.array_equal(k[f][1][0], snaps[f][i][1][0]) and np.array_equal(k[f][1][1], snaps[f][i][1][1]), (i, f)
        _same_state(a, 0, b, i, i)
        assert a.camera(0) == b.camera(i)
        a.close()
    b.close()


def test_published_points_are_the_host_lift(P):
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    kb, mei, _ = _lenses(P)
    b = P.VioBatch(cfg, 2)
    b.set_camera(0, kb)
    b.set_camera(1, mei)
    cams = [kb, mei]
    count = [0]

    def check(f, bb):
        for i in range(2):
            ids, obs = bb.packaged(i)
            if len(ids) == 0:
                continue
            _, un, _ = P.stage_host_camera(cams[i], obs[:, 3:5])
            assert np.array_equal(obs[:, 0:2], un.astype(np.float32).astype(np.float64)), (i, f)
            assert np.all(obs[:, 2] == 1.0)
            count[0] += len(ids)

    _feed(b, syn, [30, 31], lambda i, f, t: syn.render_host(30 + i, t, camera=cams[i]), 24, hook=check)
    assert count[0] > 1000
    b.close()


def test_pose_graph_keypoints_through_the_camera(P):
    import importlib
    pg = importlib.import_module("vins-rgbd-fast_amd.posegraph")
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    kb, mei, _ = _lenses(P)
    pattern = np.random.default_rng(3).integers(-15, 16, 1024).astype(np.int32)
    for cam in (kb, mei):
        g, _ = syn.render_host(12, 3.0, camera=cam)
        _, kxy, _, kn = pg.describe(cfg, g, np.zeros((0, 2), np.float32), pattern, camera=cam)
        assert len(kxy) > 100
        _, un, _ = P.stage_host_camera(cam, kxy.astype(np.float64))
        assert np.array_equal(kn, un.astype(np.float32))
        _, _, _, kp = pg.describe(cfg, g, np.zeros((0, 2), np.float32), pattern)
        assert not np.array_equal(kn, kp)   # not the configuration's pinhole


@pytest.mark.parametrize("lens", ["kb", "mei"])
def test_trajectory_accuracy_per_lens(P, lens):
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    kb, mei, _ = _lenses(P)
    cam = kb if lens == "kb" else mei
    seqs, n = [0, 1, 2, 3], 150
    b = P.VioBatch(cfg, 4)
    for i in range(4):
        b.set_camera(i, cam)
    est, gt = [[] for _ in seqs], [[] for _ in seqs]

    def rec(f, bb):
        t = float(vio_ct.frame_times(sc, n)[f])
        for i, s in enumerate(seqs):
            st = bb.status(i)
            if st.solver_flag == 1 and st.processed:
                est[i].append(bb.window(i)[cfg.window_size, :3].copy())
                gt[i].append(syn.pose(s, t)[0])

    _feed(b, syn, seqs, lambda i, f, t: syn.render_host(seqs[i], t, camera=cam), n, hook=rec)
    ates = [vio_ct.ate_rmse(np.array(e), np.array(g)) for e, g in zip(est, gt)]
    print(lens, "ATE", ates)
    for i in range(4):
        assert len(est[i]) > 100, (i, len(est[i]))
        assert ates[i] < 0.03, (lens, i, ates)
    b.close()
