"""IMU-rate odometry of the whole batch in one launch (vio_get_latest_odometry_all, vio_get_imu_rate_odometry; be_imu_rate_odometry_kernel)
against the three definitions the project already has: the scalar per-sequence getter (bit for bit), the numpy replay imu_rate_ref.py
(pinned to the oracle by test_imu_rate_cpu.py) and the oracle itself (GPU).

One S = 5 canonical handle with a 256-sample IMU ring is fed 30 frames (the four fed sequences are NON_LINEAR then, the ring has wrapped;
sequence 4 only ever sees VIO_FRAME_SKIP and stays INITIAL).  Its snapshot is taken once; every test restores it into a fresh handle, so the
tests do not depend on each other's pushes and a "twin" is a second handle restored from the same blobs."""
import importlib
import os
import sys

import numpy as np
import pytest

import imu_rate_ref
import vio_ct

pytestmark = pytest.mark.gpu

SEQS = [14, 3, 21, 40]     # synthetic sequences in slots 0 .. 3; slot 4 stays INITIAL
S, N_FRAMES, NIMU = 5, 30, 256


def _until(ti, k, tf):
    """the samples through the frame stamp and one beyond (dataio.replay's rule): exactly one sample is newer than the frame"""
    while k < len(ti) and ti[k] <= tf + 1e-9:
        k += 1
    return min(len(ti), k + 1)


class Base:
    pass


@pytest.fixture(scope="module")
def base(P):
    B = Base()
    B.cfg = P.canonical_config()
    B.sc = vio_ct.synth_like(B.cfg)
    syn = P.Synth(B.sc)
    B.times = vio_ct.frame_times(B.sc, N_FRAMES + 1)
    B.imu = [syn.imu(s, int((N_FRAMES + 1) / B.sc.cam_rate * B.sc.imu_rate) + 400) for s in SEQS]
    B.frames = [[syn.render_host(s, float(t)) for t in B.times] for s in SEQS]   # one frame more than is fed: the output-only test feeds it
    B.modes = np.array([P.FRAME_PUBLISH] * 4 + [P.FRAME_SKIP], np.uint8)
    b = P.VioBatch(B.cfg, S, imu_capacity=NIMU)
    assert b.capacity()["imu"] == NIMU
    B.k = [0] * 4
    for f in range(N_FRAMES):
        tf = float(B.times[f])
        for i in range(4):
            k2 = _until(B.imu[i][0], B.k[i], tf)
            b.push_imu(i, B.imu[i][0][B.k[i]:k2], B.imu[i][1][B.k[i]:k2], B.imu[i][2][B.k[i]:k2])
            B.k[i] = k2
        b.feed(B.gray(f), B.depth(f), [tf] * S, modes=B.modes)
    st = b.status_all()
    assert [x.solver_flag for x in st] == [1, 1, 1, 1, 0]
    assert min(B.k) > NIMU                       # the 30 frames have wrapped the ring
    B.blobs = [x.copy() for x in b.save(list(range(S)))]
    B.window = [b.window(i) for i in range(S)]
    B.td = [x.td for x in st]
    # samples newer than the window state that were pushed with the last frame (the one beyond its stamp)
    B.n0 = [int((B.imu[i][0][:B.k[i]] > B.window[i][B.cfg.window_size][16] + B.td[i]).sum()) for i in range(4)]
    assert min(B.n0) >= 1
    return B


def _gray(self, f):
    return np.stack([self.frames[i][f][0] for i in range(4)] + [self.frames[0][f][0]])


def _depth(self, f):
    return np.stack([self.frames[i][f][1] for i in range(4)] + [self.frames[0][f][1]])


Base.gray, Base.depth = _gray, _depth


def fresh(P, base):
    b = P.VioBatch(base.cfg, S, imu_capacity=NIMU)
    b.load(list(range(S)), base.blobs)
    return b


def push(b, base, i, k0, n):
    """samples k0 .. k0 + n of slot i's stream in one call"""
    t, a, g = base.imu[i]
    if n > 0:
        b.push_imu(i, t[k0:k0 + n], a[k0:k0 + n], g[k0:k0 + n])


def scalar_rows(P, base, i, n):
    """the parent's path: a twin handle gets n more samples of slot i ONE AT A TIME and is asked with latest_odometry(i) after each.
    Returns [n + 1][11]: row 0 is the answer before the first of them."""
    tw = fresh(P, base)
    out = [tw.latest_odometry(i)]
    for j in range(n):
        push(tw, base, i, base.k[i] + j, 1)
        out.append(tw.latest_odometry(i))
    tw.close()
    return np.array(out)


@pytest.fixture(scope="module")
def scalar(P, base):
    """computed once: the scalar getter's answers after each of up to 130 pending samples, per live slot"""
    return [scalar_rows(P, base, i, n) for i, n in enumerate((63, 130, 64, 65))]


def test_restored_handle_is_the_fed_one(P, base):
    b = fresh(P, base)
    for i in range(S):
        assert np.array_equal(b.window(i), base.window[i])
    assert [x.solver_flag for x in b.status_all()] == [1, 1, 1, 1, 0]


def test_prefix_property_and_bit_equality_with_the_scalar_getter(P, base, scalar):
    """pending samples 0, 1, 64, 65, then topped up to 63, 130, 64, 65 (with the one sample beyond the last frame the applied counts cross
    the 64-lane chunk on the way): row k of slot s is what latest_odometry(s) returned when the k-th sample had just arrived."""
    b = fresh(P, base)
    have = [0, 0, 0, 0]
    for want in ((0, 1, 64, 65), (63, 130, 64, 65)):
        for i in range(4):
            push(b, base, i, base.k[i] + have[i], want[i] - have[i])
            have[i] = want[i]
        n, rows = b.imu_rate_odometry(cap=160)
        all_ = b.latest_odometry_all()
        assert all_.shape == (S, 11)
        for i in range(4):
            n0 = base.n0[i]                   # samples beyond the last frame that were pushed with it
            assert n[i] == n0 + want[i], (i, n[i])
            got = rows[i, :n[i]]
            assert np.array_equal(got[n0 - 1:], scalar[i][:want[i] + 1]), (want, i)
            assert np.all(np.diff(got[:, 0]) > 0)
            assert not rows[i, n[i]:].any()                                          # nothing beyond the rows
            assert np.array_equal(all_[i], b.latest_odometry(i)) and np.array_equal(all_[i], got[-1])
        # the INITIAL slot: no rows, the window state
        assert n[4] == 0 and not rows[4].any()
        assert np.array_equal(all_[4], b.latest_odometry(4))
        w4 = base.window[4][b.status(4).frame_count]
        assert np.array_equal(all_[4], np.r_[w4[16] + base.td[4], w4[:10]])


def test_ring_wrap_and_overwrite(P, base):
    """300 pending samples into a 256-sample ring (in three pushes, each made resident by a poll): the oldest are overwritten, the 256
    survivors are all newer than the window state, and the rows end where the scalar getter ends."""
    b = fresh(P, base)
    i = 1
    for c in range(3):
        push(b, base, i, base.k[i] + 100 * c, 100)
        n, _ = b.imu_rate_odometry(cap=0)
    t_all = base.imu[i][0][:base.k[i] + 300]
    assert n.tolist() == [base.n0[0], NIMU, base.n0[2], base.n0[3], 0]
    n, rows = b.imu_rate_odometry(cap=NIMU)
    assert n[i] == NIMU
    assert np.array_equal(rows[i, :, 0], t_all[-NIMU:])
    lo = b.latest_odometry(i)
    assert np.array_equal(rows[i, NIMU - 1], lo)
    assert np.array_equal(b.latest_odometry_all()[i], lo)


def test_since_and_cap(P, base):
    b = fresh(P, base)
    for i, m in enumerate((20, 30, 64, 11)):
        push(b, base, i, base.k[i], m)
    n, rows = b.imu_rate_odometry(cap=80)
    assert n.tolist() == [base.n0[0] + 20, base.n0[1] + 30, base.n0[2] + 64, base.n0[3] + 11, 0]
    n2, rows2 = b.imu_rate_odometry(since=rows[:, 9, 0], cap=80)       # slot 4 has no row 9: its since is 0.0, and it has no rows anyway
    assert n2.tolist() == [n[0] - 10, n[1] - 10, n[2] - 10, n[3] - 10, 0]
    for i in range(4):
        assert np.array_equal(rows2[i, :n2[i]], rows[i, 10:n[i]]) and not rows2[i, n2[i]:].any()
    # a poller that has everything gets nothing
    n3, rows3 = b.imu_rate_odometry(since=[rows[i, max(n[i] - 1, 0), 0] for i in range(S)], cap=4)
    assert not n3.any() and not rows3.any()
    # cap = 4: the first four rows and the full count; what lies beyond is left untouched
    n4 = np.zeros(S, np.int32)
    rows4 = np.full((S, 4, 11), -7.0)
    rows4_guard = np.full((S, 6, 11), -7.0)
    assert b.L.vio_get_imu_rate_odometry(b.h, None, 4, n4.ctypes.data, rows4.ctypes.data, 0) == 0
    assert n4.tolist() == n.tolist()
    for i in range(4):
        assert np.array_equal(rows4[i], rows[i, :4])
    assert np.all(rows4[4] == -7.0)
    # cap = 0 only counts (out NULL)
    n0 = np.zeros(S, np.int32)
    assert b.L.vio_get_imu_rate_odometry(b.h, None, 0, n0.ctypes.data, None, 0) == 0
    assert n0.tolist() == n.tolist()
    # rows of a sequence with fewer than cap rows: the tail of its block is untouched
    n6 = np.zeros(S, np.int32)
    since = np.array([rows[i, max(n[i] - 3, 0), 0] for i in range(S)])
    assert b.L.vio_get_imu_rate_odometry(b.h, since.ctypes.data, 6, n6.ctypes.data, rows4_guard.ctypes.data, 0) == 0
    assert n6.tolist() == [2, 2, 2, 2, 0]
    for i in range(4):
        assert np.array_equal(rows4_guard[i, :2], rows[i, n[i] - 2:n[i]]) and np.all(rows4_guard[i, 2:] == -7.0)
    # argument checks
    assert b.L.vio_get_imu_rate_odometry(b.h, None, -1, n0.ctypes.data, rows4.ctypes.data, 0) == -1
    assert b.L.vio_get_imu_rate_odometry(b.h, None, 4, None, rows4.ctypes.data, 0) == -1
    assert b.L.vio_get_latest_odometry_all(b.h, None, 0) == -1


def test_on_device_output(P, base):
    b = fresh(P, base)
    for i, m in enumerate((5, 70, 0, 33)):
        push(b, base, i, base.k[i], m)
    cap = 72
    n, rows = b.imu_rate_odometry(cap=cap)
    buf = P.DeviceBuffer(S * cap * 11 * 8 + S * 11 * 8)
    buf.upload(0, np.zeros(S * cap * 11 + S * 11))
    nd = b.imu_rate_odometry(cap=cap, out=buf.ptr)
    assert np.array_equal(nd, n) and n.tolist() == [base.n0[0] + 5, base.n0[1] + 70, base.n0[2], base.n0[3] + 33, 0]
    assert np.array_equal(buf.download(0, (S, cap, 11), np.float64), rows)
    assert b.latest_odometry_all(out=buf.at(S * cap * 11 * 8)) is None
    assert np.array_equal(buf.download(S * cap * 11 * 8, (S, 11), np.float64), b.latest_odometry_all())
    assert np.array_equal(buf.download(0, (S, cap, 11), np.float64), rows)       # the neighbour was not touched
    buf.free()


def _run_one(P, cfg, base, i, n_frames=N_FRAMES):
    """a one-sequence handle (imu_capacity 256) fed slot i's frames and IMU like the base handle"""
    b = P.VioBatch(cfg, 1, imu_capacity=NIMU)
    t, a, g = base.imu[i]
    k = 0
    for f in range(n_frames):
        tf = float(base.times[f])
        k2 = _until(t, k, tf)
        b.push_imu(0, t[k:k2], a[k:k2], g[k:k2]); k = k2
        b.feed(base.frames[i][f][0][None], base.frames[i][f][1][None], [tf])
    return b, k


def test_quirk_handle(P, base):
    """reference_quirks bit 0: rows bit-equal to that handle's scalar getter (buffered samples take the front slot's values, later ones
    their own, acc_0 / gyr_0 never advance), different from the default handle's rows, and within 1e-6 of the numpy definition."""
    i, m = 2, 70
    cfg_q = P.canonical_config(reference_quirks=1)
    bq, k = _run_one(P, cfg_q, base, i)
    assert k == base.k[i] and np.array_equal(bq.window(0), base.window[i])       # the switch feeds nothing back into the estimator
    tw = P.VioBatch(cfg_q, 1, imu_capacity=NIMU)
    tw.load([0], bq.save([0]))
    t, a, g = base.imu[i]
    sc = [tw.latest_odometry(0)]
    for j in range(m):
        tw.push_imu(0, t[k + j:k + j + 1], a[k + j:k + j + 1], g[k + j:k + j + 1])
        sc.append(tw.latest_odometry(0))
    bq.push_imu(0, t[k:k + m], a[k:k + m], g[k:k + m])
    n, rows = bq.imu_rate_odometry(cap=80)
    assert n[0] == m + base.n0[i] and np.array_equal(rows[0, base.n0[i] - 1:n[0]], np.array(sc))
    assert np.array_equal(bq.latest_odometry_all()[0], sc[-1])
    b0 = fresh(P, base)
    push(b0, base, i, base.k[i], m)
    n0, rows0 = b0.imu_rate_odometry(cap=80)
    assert n0[i] == n[0] and np.array_equal(rows0[i, :, 0], rows[0, :, 0])
    assert np.linalg.norm(rows0[i, n[0] - 1, 1:4] - rows[0, n[0] - 1, 1:4]) > 1e-6
    ref, _ = imu_rate_ref.imu_rate_rows(base.window[i][cfg_q.window_size], base.td[i], [0, 0, cfg_q.g_norm], t[:k + m], a[:k + m], g[:k + m], k, 1)
    assert ref.shape == (n[0], 11)
    assert np.abs(ref[:, 0] - rows[0, :n[0], 0]).max() < 1e-12 and np.abs(ref[:, 1:] - rows[0, :n[0], 1:]).max() < 1e-6


def test_vo_handle_applies_no_sample(P, base):
    """use_imu = 0: n_rows == 0 and the window state comes back, whatever IMU was pushed"""
    cfg = P.canonical_config(fix_depth=1)
    cfg.use_imu = 0
    cfg.lk_max_level = 3
    b = P.VioBatch(cfg, 2, imu_capacity=NIMU)
    t, a, g = base.imu[0]
    for f in range(14):
        b.feed(np.stack([base.frames[0][f][0], base.frames[1][f][0]]), np.stack([base.frames[0][f][1], base.frames[1][f][1]]),
               [float(base.times[f])] * 2)
    b.push_imu(0, t[:40], a[:40], g[:40])
    n, rows = b.imu_rate_odometry(cap=8)
    assert not n.any() and not rows.any()
    all_ = b.latest_odometry_all()
    for s in range(2):
        st = b.status(s)
        w = b.window(s)[st.frame_count]
        assert np.array_equal(all_[s], b.latest_odometry(s))
        assert np.array_equal(all_[s], np.r_[w[16] + st.td, w[:10]])
    assert b.status(0).frame_count > 0


def test_against_the_numpy_definition_and_the_oracle(P, base):
    """every row of every live slot within (1e-12, 1e-6) of imu_rate_ref on the handle's own window; the last row of one slot within 1e-5
    of the oracle that was fed the same frames and samples (the bars of test_gpu_parity2's IMU-rate tests)"""
    b = fresh(P, base)
    pend = (63, 130, 64, 65)
    for i in range(4):
        push(b, base, i, base.k[i], pend[i])
    n, rows = b.imu_rate_odometry(cap=160)
    gvec = [0, 0, base.cfg.g_norm]
    for i in range(4):
        t, a, g = base.imu[i]
        m = base.k[i] + pend[i]
        ref, _ = imu_rate_ref.imu_rate_rows(base.window[i][base.cfg.window_size], base.td[i], gvec, t[:m], a[:m], g[:m], base.k[i], 0)
        assert ref.shape == (n[i], 11), (i, ref.shape, n[i])
        assert np.abs(ref[:, 0] - rows[i, :n[i], 0]).max() < 1e-12
        assert np.abs(ref[:, 1:] - rows[i, :n[i], 1:]).max() < 1e-6, (i, float(np.abs(ref[:, 1:] - rows[i, :n[i], 1:]).max()))
    i = 3
    t, a, g = base.imu[i]
    o = vio_ct.OraclePipeline(base.cfg)
    k = 0
    for f in range(N_FRAMES):
        tf = float(base.times[f])
        k2 = _until(t, k, tf)
        o.push_imu(t[k:k2], a[k:k2], g[k:k2]); k = k2
        o.feed(base.frames[i][f][0], base.frames[i][f][1], tf)
    o.push_imu(t[k:k + pend[i]], a[k:k + pend[i]], g[k:k + pend[i]])
    lo = o.latest_odometry()
    assert abs(lo[0] - rows[i, n[i] - 1, 0]) < 1e-12 and np.abs(lo[1:] - rows[i, n[i] - 1, 1:]).max() < 1e-5


def test_output_only(P, base):
    """window, status and odometry history are what they were after the polls, and the next frame gives the window of a twin that never polled"""
    b, tw = fresh(P, base), fresh(P, base)
    def state(x):
        return ([x.window(i) for i in range(S)], [bytes(s) for s in x.status_all()], [x.odometry_history(i) for i in range(S)])
    tf = float(base.times[N_FRAMES])
    for i in range(4):
        k2 = _until(base.imu[i][0], base.k[i], tf)
        for x in (b, tw):
            push(x, base, i, base.k[i], k2 - base.k[i])
    b.sync()
    s0 = state(b)
    n, rows = b.imu_rate_odometry(cap=16)
    assert n[:4].min() >= 6
    b.imu_rate_odometry(since=rows[:, 2, 0], cap=3)
    b.latest_odometry_all()
    buf = P.DeviceBuffer(S * 16 * 11 * 8)
    b.imu_rate_odometry(cap=16, out=buf.ptr)
    buf.free()
    s1 = state(b)
    for u, v in zip(s0[0] + s0[2], s1[0] + s1[2]):
        assert np.array_equal(u, v)
    assert s0[1] == s1[1]
    for x in (b, tw):
        x.feed(base.gray(N_FRAMES), base.depth(N_FRAMES), [tf] * S, modes=base.modes)
    for i in range(S):
        assert np.array_equal(b.window(i), tw.window(i)), i
        assert np.array_equal(b.latest_odometry(i), tw.latest_odometry(i)), i
    assert not np.array_equal(b.window(0), s0[0][0])     # the frame was processed


REPLAY_YAML = """%YAML:1.0
imu: 1
static_init: 1
depth_min_dist: 0.3
depth_max_dist: 10
frontend_freq: 30
num_grid_rows: 5
num_grid_cols: 6
model_type: PINHOLE
image_width: 640
image_height: 480
distortion_parameters:
   k1: 0.0
   k2: 0.0
   p1: 0.0
   p2: 0.0
projection_parameters:
   fx: 430.0
   fy: 430.0
   cx: 320.0
   cy: 240.0
estimate_extrinsic: 0
max_cnt: 150
min_dist: 25
freq: 10
F_threshold: 1.0
max_num_iterations: 8
keyframe_parallax: 10.0
acc_n: 0.1
gyr_n: 0.01
acc_w: 0.001
gyr_w: 0.0001
g_norm: 9.805
estimate_td: 0
td: 0.0
rolling_shutter: 0
"""


def test_replay_writes_the_imu_rate_stream(P, tmp_path):
    """tools/replay.py --imu-rate-out on a written 30 Hz synthetic recording (freq 10 / frontend_freq 30, as test_gpu_replay.py): strictly
    ascending stamps, one row per IMU sample from the moment the estimator is NON_LINEAR, and the last row written before each frame is
    latest_odometry taken at that point (bit for bit in the process, to the file's 5 decimals in the file)."""
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    cfg, extra = io.config_from_yaml(REPLAY_YAML, P)
    sc = vio_ct.synth_like(cfg, cam_rate=30.0)
    syn = P.Synth(sc)
    seq, n = 6, 48
    stamps = vio_ct.frame_times(sc, n)
    frames = [syn.render_host(seq, float(t)) for t in stamps]
    ti, ai, gi = syn.imu(seq, int(n / sc.cam_rate * sc.imu_rate) + 64)
    io.write_recording(str(tmp_path / "rec"), stamps, [f[0] for f in frames], [f[1] for f in frames], ti, ai, gi)
    (tmp_path / "vio.yaml").write_text(REPLAY_YAML)
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        replay_tool = importlib.import_module("replay")
    finally:
        sys.path.remove(tools)
    out, fast = str(tmp_path / "vins_result.csv"), str(tmp_path / "imu_rate.csv")
    replay_tool.main(["--config", str(tmp_path / "vio.yaml"), "--data", str(tmp_path / "rec"), "--out", out, "--imu-rate-out", fast])
    rows = io.read_odometry_csv(fast)
    assert len(rows) >= 40 and np.all(np.diff(rows[:, 0]) > 0)
    # the same replay in the process, with the scalar getter asked right before every frame
    rec = io.RgbdImuDirectory(str(tmp_path / "rec"))
    b = P.VioBatch(cfg, 1, imu_capacity=1 << 15)
    wr = io.ImuRateCsvWriter(str(tmp_path / "imu_rate_2.csv"))
    seen = []
    def before(f, batch):
        lo = batch.latest_odometry(0)
        if batch.status(0).solver_flag == 1:
            assert np.array_equal(wr.last_row, lo), f
            seen.append(lo)
    io.replay(b, rec, freq=extra["freq"], frontend_freq=extra["frontend_freq"], imu_rate=wr, before_feed=before)
    wr.close()
    assert len(seen) >= 5 and wr.n == len(rows)
    dt = np.diff(rows[:, 0])
    assert abs(np.median(dt) - 1.0 / sc.imu_rate) < 1e-6                              # IMU rate, not frame rate
    for lo in seen:
        j = int(np.argmin(np.abs(rows[:, 0] - lo[0])))
        assert abs(rows[j, 0] - lo[0]) < 2e-9 and np.abs(rows[j, 1:] - lo[1:]).max() <= 5.1e-6
