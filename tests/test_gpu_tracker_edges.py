"""The tracker bookkeeping kernels (fe_begin / fe_select / fe_fast / fe_add, csrc/fe_kernels.hip) on the generated streams of
tests/tracker_cases.py against the oracle, after every frame and bit for bit: ids, track_cnt, pixel / normalised positions and velocities as
uint32, the packaged feature map, n_tracks.  No tolerance anywhere: these kernels are integer and mask logic followed by the oracle's float
operations one by one.  That every stream reaches the branch it is named for is proved on the oracle in test_tracker_cases_cpu.py."""
import numpy as np
import pytest

import tracker_cases as TC
import vio_ct

pytestmark = pytest.mark.gpu

EYE = np.eye(3)


def _state(b, i):
    st = b.status(i)
    return dict(tracks=tuple(a.copy() for a in b.tracks(i)), packaged=b.packaged(i), n_tracks=int(st.n_tracks), overflow=int(st.overflow_flags))


def _same(a, q, where):
    """a, q: dicts of tracks (ids, track_cnt, cur, un, vel), packaged (ids, obs); everything identical, floats compared as bit patterns"""
    ta, tq = a["tracks"], q["tracks"]
    assert len(ta[0]) == len(tq[0]), (where, len(ta[0]), len(tq[0]))
    assert np.array_equal(ta[0], tq[0]), (where, "ids")
    assert np.array_equal(ta[1], tq[1]), (where, "track_cnt")
    for k, what in ((2, "cur"), (3, "un"), (4, "vel")):
        assert np.array_equal(ta[k].view(np.uint32), tq[k].view(np.uint32)), (where, what)
    assert np.array_equal(a["packaged"][0], q["packaged"][0]), (where, "packaged ids")
    assert np.array_equal(a["packaged"][1].view(np.uint64), q["packaged"][1].view(np.uint64)), (where, "packaged obs")
    if "n_tracks" in q:
        assert q["n_tracks"] == len(ta[0]), (where, "n_tracks")


def run_hip(P, case):
    """the case alone on a one-sequence handle: the state after every frame"""
    b = P.VioBatch(case.cfg, 1)
    if case.fisheye is not None:
        b.set_fisheye_mask(case.fisheye)
    out = []
    for g, t, m in zip(case.frames, case.stamps, case.modes):
        b.track(g[None], [t], modes=[m], R_rel=EYE[None])
        out.append(_state(b, 0))
    b.close()
    return out


_solo = {}


def _solo_run(P, name):
    if name not in _solo:
        _solo[name] = run_hip(P, TC.build(name, P))
    return _solo[name]


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_matches_the_oracle_bit_for_bit(P, name):
    case, recs = TC.oracle_run(name, P)
    hip = _solo_run(P, name)
    assert len(recs) == len(hip) == len(case.frames)
    for f, (r, q) in enumerate(zip(recs, hip)):
        _same(r, q, (name, f))
        if len(r["track_out"][0]):    # what Pipeline::track handed on, once the nodelet's init_pub / init_feature let it through
            assert np.array_equal(r["track_out"][0], q["packaged"][0]) and np.array_equal(r["track_out"][1], q["packaged"][1]), (name, f)
        if name != "fast_overflow":
            assert q["overflow"] == 0, (name, f, q["overflow"])
    assert sum(len(q["packaged"][0]) for q in hip) > 0, name


def test_fast_overflow_flags_truncates_and_keeps_min_dist(P):
    """the noise frame gives 4843 FAST survivors for a buffer of 1024: flag 4 on that frame and on no other, the state is the oracle's with the
    same truncation (first 1024 in raster order) on that frame and after it, and the truncated selection still respects the min_dist disks"""
    case, recs = TC.oracle_run("fast_overflow", P)
    assert case.fast_cap == 1024 and recs[2]["trace"]["cells"][0]["n_fast"] > 1024
    hip = _solo_run(P, "fast_overflow")
    assert [q["overflow"] & 4 for q in hip] == [0, 0, 4, 0, 0]
    for f in (2, 3, 4):
        _same(recs[f], hip[f], ("fast_overflow", f))
    free = TC.run_oracle(case, fast_cap=0)
    assert not np.array_equal(free[2]["tracks"][2], hip[2]["tracks"][2])          # the untruncated detector keeps other points: the cap is what is tested
    r = case.cfg.min_dist
    hw = np.zeros(r + 1, np.int32)
    vio_ct.oracle().ovio_circle_hw(r, hw.ctypes.data)
    p = np.rint(hip[2]["tracks"][2]).astype(np.int64)
    assert len(p) >= 100
    dx, dy = np.abs(p[:, None, 0] - p[None, :, 0]), np.abs(p[:, None, 1] - p[None, :, 1])
    inside = (dy <= r) & (dx <= hw[np.minimum(dy, r)])
    np.fill_diagonal(inside, False)
    assert not inside.any(), np.argwhere(inside)[:4]


def test_batch_of_offset_streams_equals_the_solo_runs(P):
    """four streams of one configuration as the sequences of one handle, their starts offset: in launch 2 sequence 0 is saturated (no detection),
    sequence 1 sees its first image, sequence 2 is on a SKIP frame and sequence 3 overflows the FAST buffer.  Every sequence equals its solo
    run, and the stream with the SKIP frame the oracle, bit for bit; flags stay with their sequence."""
    skip = TC.build("unstable", P)
    skip.modes[1] = TC.SKIP
    streams = [(TC.build("serial_topk", P), 0), (TC.build("serial_addpoints", P), 2), (skip, 1), (TC.build("fast_overflow", P), 0)]
    cfg = streams[0][0].cfg
    for c, _ in streams:
        assert bytes(c.cfg) == bytes(cfg) and c.fisheye is None
    solo = [_solo_run(P, "serial_topk"), _solo_run(P, "serial_addpoints"), run_hip(P, skip), _solo_run(P, "fast_overflow")]
    orc = TC.run_oracle(skip)
    assert len(orc) == len(solo[2]) == len(skip.frames)
    for f, (r, q) in enumerate(zip(orc, solo[2])):
        _same(r, q, ("unstable with a SKIP frame", f))
    assert TC.oracle_run("serial_topk", P)[1][2]["trace"]["n_max_cnt"] <= 0
    n_launch = max(len(c.frames) + off for c, off in streams)
    S = len(streams)
    b = P.VioBatch(cfg, S)
    seen = [0] * S
    for k in range(n_launch):
        gray, modes, stamps = [], [], []
        for c, off in streams:
            f = k - off
            live = 0 <= f < len(c.frames)
            gray.append(c.frames[f] if live else TC.flat(cfg.width, cfg.height))
            modes.append(c.modes[f] if live else TC.SKIP)
            stamps.append(c.stamps[f] if live else TC.T0 + TC.DT * k)
        if k == 2:
            assert modes == [TC.PUBLISH, TC.PUBLISH, TC.SKIP, TC.PUBLISH]
        b.track(np.stack(gray), stamps, modes=modes, R_rel=np.stack([EYE] * S))
        for i, (c, off) in enumerate(streams):
            f = k - off
            if 0 <= f < len(c.frames):
                q = _state(b, i)
                _same(solo[i][f], q, (c.name, "launch", k))
                assert q["overflow"] == solo[i][f]["overflow"] == (4 if (i, f) == (3, 2) else 0), (c.name, k)
                seen[i] += 1
    assert seen == [len(c.frames) for c, _ in streams]
    b.close()


def test_refused_configurations(P):
    """what build_devcfg turns away around the tracker's buffers: a track capacity beyond the FAST candidate buffer, no feature per cell"""
    for kw in (dict(max_cnt=600), dict(rows=8, cols=8, max_cnt=60)):
        with pytest.raises(P.VioError):
            P.VioBatch(TC.config(P, **kw), 1)
