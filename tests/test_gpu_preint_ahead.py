"""VIO_PREINT_AHEAD: vio_feed pre-integrates a frame's IMU interval beside be_marg of the previous frame (be_preint_ahead_kernel) and be_ingest takes
the result over where every input still has the bits it would use itself.  Same device functions, same operands, so a handle created with
VIO_PREINT_AHEAD=1 must expose the same BITS as one created with =0 on identical input: window, odometry row, every vio_status field and the
vio_save_seqs blob of every sequence after EVERY frame -- and vio_debug_preint_ahead must show that the staged path was really taken.

S = 3 sequences of 640 x 480 images, window_size 4 (the smallest window of the back-end tests).  Sequence 0 never moves (every slide is
MARGIN_SECOND_NEW), the others start moving right after the static initialisation (MARGIN_OLD once the parallax is there).  Reading a handle
after every frame waits for it, so the new kernel then never really runs beside be_marg; test_frames_queued_ahead_of_the_device feeds the same
frames back to back and compares the end state and the odometry history."""
import numpy as np
import pytest

import vio_ct

pytestmark = pytest.mark.gpu

W = 4
VIO_NEED_IMU = 1
KNOBS = ("VIO_PREINT_AHEAD", "VIO_GROUP_SEQS")

_frames, _imu = {}, {}


def _cfg(P, **kw):
    return P.canonical_config(window_size=W, **kw)


def _scenes(cfg, cam_rate=5.0):
    """(still, moving): the same rig; `still` never leaves its static phase, `moving` leaves it when the static initialisation has its W + 1 frames"""
    still = vio_ct.synth_like(cfg, cam_rate=cam_rate, t_static=1e3)
    moving = vio_ct.synth_like(cfg, cam_rate=cam_rate, t_static=W / cam_rate)
    return still, moving


def _rendered(P, sc, seq, tf):
    key = (bytes(sc), seq, float(tf))
    if key not in _frames:
        _frames[key] = P.Synth(sc).render_host(seq, float(tf))
    return _frames[key]


def _imu_of(P, sc, seq, t_end):
    key = (bytes(sc), seq)
    n = int(t_end * sc.imu_rate) + 64
    if key not in _imu or len(_imu[key][0]) < n:
        _imu[key] = P.Synth(sc).imu(seq, n)
    return _imu[key]


def _status(st):
    return {k: getattr(st, k) for k, _ in st._fields_}


def _record(b):
    S = b.S
    return dict(status=[_status(st) for st in b.status_all()], window=[b.window(i).copy() for i in range(S)], odo=b.odometry().copy(),
                blobs=[x.copy() for x in b.save(list(range(S)))], stats=b.preint_ahead_stats(per_seq=True).copy())


def _same(a, r, f):
    for i, (sa, sr) in enumerate(zip(a["status"], r["status"])):
        assert sa == sr, (f, i, sa, sr)
    for i, (wa, wr) in enumerate(zip(a["window"], r["window"])):
        assert np.array_equal(wa.view(np.uint64), wr.view(np.uint64)), (f, i, float(np.abs(wa - wr).max()))
    assert np.array_equal(a["odo"].view(np.uint64), r["odo"].view(np.uint64)), f
    for i, (ba, br) in enumerate(zip(a["blobs"], r["blobs"])):
        assert ba.size == br.size and np.array_equal(ba, br), (f, i, int(np.count_nonzero(ba != br)) if ba.size == br.size else -1)


class Run:
    """One handle fed frame by frame.  seqs = [(scene, synthetic sequence)], times = the frame stamps; feed(f, hold=(i,)) keeps back the IMU of
    the listed slots for that frame (it goes in with the next frame's)."""

    def __init__(self, P, monkeypatch, cfg, seqs, times, ahead, lag=1, group=None, lead=None):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("VIO_PREINT_AHEAD", str(int(ahead)))
        if group is not None:
            monkeypatch.setenv("VIO_GROUP_SEQS", str(group))
        self.P, self.seqs, self.times = P, seqs, [float(t) for t in times]
        self.b = P.VioBatch(cfg, len(seqs))
        if lag:
            self.b.set_tracker_lag(lag)
        self.imu = [_imu_of(P, sc, s, self.times[-1]) for sc, s in seqs]
        self.k = [0] * len(seqs)
        self.lead = lead      # seconds of IMU pushed beyond a frame's stamp (None: vio_ct.imu_until's sample and a half)

    def feed(self, f, hold=()):
        tf = self.times[f]
        for i, (ti, ai, gi) in enumerate(self.imu):
            if i in hold:
                continue
            k2 = vio_ct.imu_until(ti, self.k[i], tf, self.seqs[i][0].imu_rate) if self.lead is None else int(np.searchsorted(ti, tf + self.lead))
            if k2 > self.k[i]:
                self.b.push_imu(i, ti[self.k[i]:k2], ai[self.k[i]:k2], gi[self.k[i]:k2])
            self.k[i] = k2
        fr = [_rendered(self.P, sc, s, tf) for sc, s in self.seqs]
        self.b.feed(np.stack([x[0] for x in fr]), np.stack([x[1] for x in fr]), [tf] * len(self.seqs))

    def run(self, frames, hold=None):
        out = []
        for f in frames:
            self.feed(f, (hold or {}).get(f, ()))
            out.append(_record(self.b))
        return out


def _pair(P, monkeypatch, cfg, seqs, times, **kw):
    hold = kw.pop("hold", None)
    ref = Run(P, monkeypatch, cfg, seqs, times, 0, **kw).run(range(len(times)), hold)
    alt = Run(P, monkeypatch, cfg, seqs, times, 1, **kw).run(range(len(times)), hold)
    for f, (a, r) in enumerate(zip(alt, ref)):
        _same(a, r, f)
        assert not r["stats"].any(), f                      # VIO_PREINT_AHEAD=0: nothing is ever staged
    return ref, alt


def _used(alt, f, i):
    return int(alt[f]["stats"][i, 0] - (alt[f - 1]["stats"][i, 0] if f else 0))


def _declined(alt, f, i):
    return int(alt[f]["stats"][i, 1] - (alt[f - 1]["stats"][i, 1] if f else 0))


def _check_use(ref, alt, skip=()):
    """the staged result is used in every steady frame (NON_LINEAR with a full window since before the previous frame's slide) and in none while
    the sequence was INITIAL after the previous frame; returns the steady frames per sequence"""
    steady = []
    for i in range(len(ref[0]["status"])):
        mine = []
        for f in range(2, len(ref)):
            if (f, i) in skip:
                continue
            before, prev, now = ref[f - 2]["status"][i], ref[f - 1]["status"][i], ref[f]["status"][i]
            if prev["solver_flag"] == 0:
                assert _used(alt, f, i) == 0, (f, i)
            elif before["solver_flag"] == 1 and now["processed"] and now["reboot_count"] == before["reboot_count"]:
                assert prev["frame_count"] == W
                assert _used(alt, f, i) == 1 and _declined(alt, f, i) == 0, (f, i, _used(alt, f, i), _declined(alt, f, i))
                mine.append(f)
        steady.append(mine)
    return steady


def _canonical_plan(P, cfg, n_seq=3, n=W + 16):
    still, moving = _scenes(cfg)
    return [(still, 60)] + [(moving, 61 + i) for i in range(n_seq - 1)], vio_ct.frame_times(moving, n)


@pytest.mark.parametrize("lag", [1, 0])
def test_steady_state_takes_the_staged_result_over(P, monkeypatch, lag):
    cfg = _cfg(P)
    seqs, times = _canonical_plan(P, cfg)
    ref, alt = _pair(P, monkeypatch, cfg, seqs, times, lag=lag)
    steady = _check_use(ref, alt)
    assert all(len(m) >= 8 for m in steady), steady
    assert all(r["solver_flag"] == 1 for r in ref[-1]["status"]), ref[-1]["status"]
    # a stretch in which sequence 0 slides MARGIN_SECOND_NEW while the others slide MARGIN_OLD
    mixed = [f for f in steady[0] if ref[f]["status"][0]["marginalization_flag"] == 1 and
             all(ref[f]["status"][i]["marginalization_flag"] == 0 for i in (1, 2))]
    assert mixed, [[r["status"][i]["marginalization_flag"] for i in range(3)] for r in ref]


def test_frames_queued_ahead_of_the_device(P, monkeypatch):
    """no read between the feeds: be_preint_ahead_kernel of frame f is queued while be_marg of frame f - 1 has not run yet"""
    cfg = _cfg(P)
    seqs, times = _canonical_plan(P, cfg)
    end = []
    for ahead in (0, 1):
        r = Run(P, monkeypatch, cfg, seqs, times, ahead)
        for f in range(len(times)):
            r.feed(f)
        end.append((_record(r.b), [r.b.odometry_history(i).copy() for i in range(3)]))
    _same(end[1][0], end[0][0], len(times) - 1)
    for i in range(3):
        assert np.array_equal(end[1][1][i].view(np.uint64), end[0][1][i].view(np.uint64)), i
    # every frame behind the first NON_LINEAR one is steady (the first may or may not see the flag that be_marg sets beside it)
    nl = [int(st["frames_processed"]) - (W + 1) for st in end[0][0]["status"]]
    assert all(n >= 8 for n in nl), nl
    assert all(end[1][0]["stats"][i, 0] >= nl[i] - 1 for i in range(3)), (end[1][0]["stats"], nl)


def test_two_stream_groups(P, monkeypatch):
    cfg = _cfg(P)
    seqs, times = _canonical_plan(P, cfg, n_seq=4, n=W + 12)
    ref, alt = _pair(P, monkeypatch, cfg, seqs, times, group=2)
    steady = _check_use(ref, alt)
    assert all(len(m) >= 4 for m in steady), steady


def test_time_offset_estimated(P, monkeypatch):
    """estimate_td = 1: curTime = stamp + td depends on the previous solve.  Three moving sequences (td cannot be observed at rest: the still
    sequence's estimate runs away within a few frames of this short window), and 50 ms of IMU beyond every stamp so that stamp + td stays covered."""
    cfg = _cfg(P, estimate_td=1)
    _, moving = _scenes(cfg)
    seqs, times = [(moving, 61), (moving, 62), (moving, 63)], vio_ct.frame_times(moving, W + 16)
    ref, alt = _pair(P, monkeypatch, cfg, seqs, times, lead=0.05)
    steady = _check_use(ref, alt)
    assert all(len(m) >= 1 for m in steady) and sum(len(m) for m in steady) >= 8, steady
    assert any(r["status"][i]["td"] != 0.0 for r in ref for i in range(3)), "td never moved: the case does not test what it is here for"


def test_late_imu(P, monkeypatch):
    """sequence 1 gets the IMU of one steady frame only after the feed that needed it: VIO_NEED_IMU and a declined record on that frame, the staged
    path again from the next one"""
    cfg = _cfg(P)
    seqs, times = _canonical_plan(P, cfg)
    late = W + 10
    ref, alt = _pair(P, monkeypatch, cfg, seqs, times, hold={late: (1,)})
    assert ref[late]["status"][1]["code"] == VIO_NEED_IMU and not ref[late]["status"][1]["processed"], ref[late]["status"][1]
    assert _used(alt, late, 1) == 0 and _declined(alt, late, 1) == 1
    # (the next frame carries both intervals: 80 samples, more than a slot's buffers hold -- overflow bit 2, by the staged path's own rule)
    assert ref[late + 1]["status"][1]["processed"] and ref[late + 1]["status"][1]["overflow_flags"] & 2, ref[late + 1]["status"][1]
    steady = _check_use(ref, alt, skip={(late, 1)})
    assert late + 1 in steady[1] and late + 2 in steady[1], steady
    assert late in steady[0] and late in steady[2], steady


def test_interval_lengths(P, monkeypatch):
    """frames that carry n = 1, PI_CH + 1 = 9 and VIO_IMU_SLOT_CAP + 1 = 65 IMU samples (200 Hz; the stamps lie 1 ms off the IMU grid).  The rig holds
    still, so the long gap costs no tracks.  The run ends with the 65-sample frame: on the frames behind that gap two runs of the SAME handle kind
    already differ in the solver's scratch record (the sst row of a blob), so there is no reference to compare with."""
    cfg = _cfg(P)
    still, _ = _scenes(cfg, cam_rate=10.0)
    seqs = [(still, 60), (still, 61), (still, 62)]
    times = [0.001 + 0.1 * j for j in range(W + 6)]
    for gap in (0.002, 0.040, 0.320):
        times.append(times[-1] + gap)
    ti = _imu_of(P, still, 60, times[-1])[0]
    n_of = [None] + [int(np.searchsorted(ti, b, "left") - np.searchsorted(ti, a, "right") + 1) for a, b in zip(times[:-1], times[1:])]
    assert n_of[W + 6:W + 9] == [1, 9, 65], n_of
    ref, alt = _pair(P, monkeypatch, cfg, seqs, times)
    steady = _check_use(ref, alt)
    assert all({W + 6, W + 7, W + 8} <= set(m) for m in steady), steady
    for i in range(3):
        assert ref[W + 8]["status"][i]["overflow_flags"] & 2, ref[W + 8]["status"][i]            # 65 samples: one past the slot's buffers
        assert not ref[W + 7]["status"][i]["overflow_flags"] & 2 and not ref[W + 6]["status"][i]["overflow_flags"] & 2


def test_snapshots_cross_between_the_two_kinds_of_handle(P, monkeypatch):
    """saved from a VIO_PREINT_AHEAD=1 handle in mid steady state, loaded into a fresh =0 handle, and the reverse: four more frames equal an
    uninterrupted run (the records are not part of a snapshot; a restored handle starts without one)"""
    cfg = _cfg(P)
    seqs, times = _canonical_plan(P, cfg)
    cut = W + 10
    ref = Run(P, monkeypatch, cfg, seqs, times, 0).run(range(cut + 4))
    for src_kind in (1, 0):
        a = Run(P, monkeypatch, cfg, seqs, times, src_kind)
        head = a.run(range(cut))
        _same(head[-1], ref[cut - 1], cut - 1)
        c = Run(P, monkeypatch, cfg, seqs, times, 1 - src_kind)
        c.b.load([0, 1, 2], head[-1]["blobs"])
        c.k = list(a.k)
        tail = c.run(range(cut, cut + 4))
        for f, rec in zip(range(cut, cut + 4), tail):
            _same(rec, ref[f], f)
        if src_kind == 0:
            assert (tail[-1]["stats"][:, 0] >= 3).all(), tail[-1]["stats"]   # (the first feed of a handle has no earlier solve to wait for)
        else:
            assert not tail[-1]["stats"].any()
