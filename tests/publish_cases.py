"""The streams the publisher tests run (tests/test_publish_ref_cpu.py on the oracle, tests/test_gpu_publish.py on the handle): the streams of
tests/backend_cases.py that between them reach the branches of publish_ref.BRANCHES, and the streams of this file for the branches none
of those reaches.

starved: a moving stream in which the IMU samples of frame 9 are held back until after the frame was offered: processImage finds the IMU short
of the stamp and returns without consuming anything (estimator.cpp:178-183; VIO_NEED_IMU), the frame is offered again with its samples.  The
publishers see an unprocessed frame on a NON_LINEAR sequence.

w20_late: window_size 20, every moving frame a keyframe, and six landmarks that first appear on frame W + 3 and stay for eight frames: they
start in window frame 20 and come down one frame per slide, so that with two and more observations they start in frames 17 and 16, beyond
3 W / 4 = 15 and below W - 2: the one window size at which pubPointCloud's start_frame > WINDOW_SIZE * 3.0 / 4.0 test can bite."""
import numpy as np

import backend_cases as BC
import publish_ref as PR

STREAMS = ("short_tracks", "depth_edges", "reappear", "thin", "standstill", "w10_td", "w20_moving", "vo_depthless", "vo_half_turn", "starved", "w20_late")
STARVED_FRAME = 9
_built = {}


def starved(P):
    cfg, sc, stamps = BC._moving(P, 16)
    st = BC.Stream("starved", cfg, sc, stamps, about="a frame offered before its IMU samples: not processed, then offered again")
    st.notes["starved"] = STARVED_FRAME
    return st


def w20_late(P):
    W = 20
    cfg, sc, stamps = BC._moving(P, W + 14, window_size=W, speed=2.5)
    return BC.Stream("w20_late", cfg, sc, stamps, hooks=[BC.show_extras({W + 3: [(0, 6, 8)]})], about="landmarks that start beyond 3 W / 4")


OWN = dict(starved=starved, w20_late=w20_late)


def build(name, P):
    if name in OWN:
        if name not in _built:
            _built[name] = OWN[name](P)
            _built[name].frames()
        return _built[name]
    if name == "w20_moving":
        return BC.w20_moving(P)
    if name in BC.VO_CASES:
        return BC.build_vo(name, P)
    return BC.build(name, P)


def offers(st):
    """the stream as a list of offers (stamp, ids, obs, depth, imu, expect_processed): the frames of st.frames(), with the starved frame
    offered once without its IMU samples first"""
    out = []
    empty = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)))
    for k, (stamp, ids, obs, depth, imu) in enumerate(st.frames()):
        if st.notes.get("starved") == k:
            out.append((stamp, ids, obs, depth, empty, False))
        out.append((stamp, ids, obs, depth, imu, True))
    return out


def run_oracle(st, taken=None):
    """the oracle over the offers: per offer dict(processed, status, window, lm, extrinsic, out = publish_ref.publish(...)); taken collects
    the branches"""
    import vio_ct
    o = vio_ct.OraclePipeline(st.cfg)
    W = st.cfg.window_size
    mirror, recs = PR.TrackMirror(W, st.cfg.depth_min), []
    for stamp, ids, obs, depth, (ti, ai, gi), expect in offers(st):
        if len(ti):
            o.push_imu(ti, ai, gi)
        processed = int(o.process_obs(ids, obs, BC.oracle_depth(depth), stamp))
        assert bool(processed) == expect, (st.name, stamp, processed)
        status = dict(o.status(), processed=processed)
        lm, window, ex = o.landmarks_ex().copy(), o.window().copy(), np.zeros(13)
        vio_ct.oracle().ovio_get_extrinsic(o.h, ex.ctypes.data)
        if processed:
            mirror.frame(ids, obs, lm, status["marginalization_flag"], depth)
        out = PR.publish(lm, window, ex, status, mirror.fed_at(lm, window, W - 2), taken=taken)
        recs.append(dict(processed=processed, status=status, window=window, lm=lm, extrinsic=ex, out=out))
    return recs
