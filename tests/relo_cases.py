"""Relocalisation requests (vio_set_relo_frame / Estimator::setReloFrame) on the generated streams of tests/backend_cases.py, placed so that
the latch, the factor selection of solve_prologue and the solve that carries the factors reach their structural edges.

A case is a stream plus a list of requests.  A request names the frame after which it is made and how its arguments are derived: the stamp is
that of window slot `index` (or one that is in no window), the "old keyframe" is the stream frame `back` frames before that slot's frame, its
pose is the scene's truth there, and its match points are the union of the observations of the stream frames from the old frame up to the
request frame, keyed by id and ascending (an old keyframe that saw everything); `select` then thins that list.  resolve() turns a request
into the arguments of set_relo_frame from a pipeline's window and landmark table; drive() runs a case over any pipeline through accessors
and hands the resolved arguments back, so that a second pipeline can be given the very same request.

tests/test_relo_cases_cpu.py shows on the oracle alone that every case reaches the branch it is named for,
tests/test_gpu_relo_edges.py compares the HIP back end with the oracle on them."""
import numpy as np

import backend_cases as BC

UNKNOWN_STAMP = 123.456      # in no window of any stream here
FRAME_INDEX = 7              # the pose graph's index of the matched frame: stored, never read by the back end
ABSENT_ID = 10_000_000       # beyond every stream's next_id


class Request:
    """after: the stream frame after which the request is made; index: the window slot whose stamp it names; back: the old frame lies
    `back` stream frames before that slot's frame; select: how the match list is thinned (resolve); unknown: the stamp is UNKNOWN_STAMP
    instead (everything else is still derived from slot `index`); yaw_deg: the old keyframe's pose turned about the world's z axis"""

    def __init__(self, after, index, back=3, select="all", unknown=False, yaw_deg=0.0, count=0):
        self.after, self.index, self.back, self.select, self.unknown, self.yaw_deg, self.count = after, index, back, select, unknown, yaw_deg, count


class Case:
    def __init__(self, name, stream, requests, about):
        self.name, self.stream, self.requests, self.about = name, stream, list(requests), about
        self.cfg = stream.cfg


# ------------------------------------------------------------------------------------------------------------- streams
def spread(P, name="relo_spread"):
    """every moving frame a keyframe; extras appear on frames 12 .. 16, four per frame, and stay for 8 frames: when the request is made after
    frame 17 the window holds in-problem landmarks that start in slot 0 and in slot 1"""
    cfg, sc, stamps = BC._moving(P, 24, speed=2.5)
    plan = {12: [(0, 4, 8)], 13: [(4, 4, 8)], 14: [(8, 4, 8)], 15: [(12, 4, 8)], 16: [(16, 4, 8)]}
    return BC.Stream(name, cfg, sc, stamps, hooks=[BC.show_extras(plan)])


def sparse_ids(P):
    """landmark j under id 1000 (j + 1): room for a whole match list of absent ids between two landmarks"""
    cfg, sc, stamps = BC._moving(P, 22, speed=2.5)
    st = BC.Stream("relo_sparse_ids", cfg, sc, stamps)
    st.ids_of[:sc.n_base] = 1000 * (1 + np.arange(sc.n_base))
    st.next_id = 100000
    return st


def hold(P):
    """_standstill with a hold of 6 frames: frames W + 4 .. W + 8 are non-keyframes, the frames after the hold are keyframes again"""
    return BC._standstill("relo_hold", P, 6, "a request after a non-keyframe and after a keyframe")


def td_stream(P):
    """w10_td's stamps and motion with td estimated and the extrinsic fixed: the td column sits beside the lent extrinsic block"""
    W = 10
    cfg = BC.case_config(P, window_size=W, estimate_td=1, estimate_extrinsic=0)
    s1 = BC._stamps(W + 1 + 3, 2.0)
    rest = s1[-1] + 0.5 * np.arange(1, W + 6)
    stamps = np.concatenate([s1, rest])
    sc = BC.CaseScene(cfg, [(stamps[W], stamps[-1] + 2.0, 1.0)], 50.0)
    return BC.Stream("relo_td", cfg, sc, stamps)


def wide(P, W, n):
    cfg, sc, stamps = BC._moving(P, n, window_size=W)
    return BC.Stream("relo_w%d" % W, cfg, sc, stamps)


def vo_stream(P):
    cfg, sc, stamps = BC._moving(P, 18, fix_depth=1, depth_max=10.0)
    cfg.use_imu = 0
    return BC.Stream("relo_vo", cfg, sc, stamps)


F_SPREAD = 17        # the spread stream's request frame
CASES = {
    "index_0": (spread, [Request(F_SPREAD, 0)], "slot 0, the frame about to be marginalised: its old frame lies outside the window; the start filter bites"),
    "index_1": (spread, [Request(F_SPREAD, 1)], "slot 1: landmarks that start in slot 1 pass the start filter"),
    "index_Wm2": (spread, [Request(F_SPREAD, 2)], "slot W - 2"),
    "index_Wm1": (spread, [Request(F_SPREAD, 3)], "slot W - 1, the last one setReloFrame looks at"),
    "no_overlap": (spread, [Request(F_SPREAD, 1, select="absent")], "every match id beyond next_id: zero factors, a zero Hessian in the lent block"),
    "empty": (spread, [Request(F_SPREAD, 1, select="empty")], "n = 0 with a NULL match pointer"),
    "single": (spread, [Request(F_SPREAD, 1, select="first", count=1)], "one factor: two residual rows for six degrees of freedom"),
    "ends": (sparse_ids, [Request(14, 1, select="ends")], "two matched ids, first and last of a match list of tracker-capacity length"),
    "not_in_problem": (spread, [Request(F_SPREAD, 0, select="not_in_problem")], "ids in the table, none of them a factor"),
    "after_keyframe": (hold, [Request(16, 1)], "a request after a MARGIN_OLD frame: the copied pose is one slot older (upstream's quirk)"),
    "after_non_keyframe": (hold, [Request(10, 1)], "a request after the first MARGIN_SECOND_NEW frame of the hold (its marginalisation re-runs "
                           "vector2double: the prior still holds pose W - 1): the copy is exact"),
    "after_second_non_keyframe": (hold, [Request(11, 1)], "after the next one (the prior no longer holds pose W - 1, no vector2double): the copy is "
                                  "the pose as the solve left it, before double2vector's gauge fix"),
    "superseded_a": (spread, [Request(F_SPREAD, 1), Request(F_SPREAD, 2, back=2)], "two requests before one solve, both stamps in the window: the second wins"),
    "superseded_b": (spread, [Request(F_SPREAD, 1), Request(F_SPREAD, 2, back=2, select="first", count=5, unknown=True)],
                     "the second stamp unknown: the first index stays latched with the second's match points and pose"),
    "during_init": (spread, [Request(2, 1)], "a request while solver_flag == 0: it waits for the solve that ends the initialisation"),
    "big_yaw": (spread, [Request(F_SPREAD, 1, yaw_deg=179.5)], "the old keyframe's world turned 179.5 degrees about z"),
    "bound": (BC.depth_edges, [Request(10, 2)], "the relocalisation solve itself runs the projected line search with a bounded landmark"),
    "td": (td_stream, [Request(23, 6)], "window 10 with td estimated and active since frame 21"),
    "w11": (lambda P: wide(P, 11, 26), [Request(20, 6)], "window 11"),
    "w20": (lambda P: wide(P, 20, 36), [Request(30, 12)], "window 20: the streaming solver"),
    "vo": (vo_stream, [Request(10, 1)], "VO mode: the literal reference carries the factors, the HIP path drops the request (DESIGN.md section 4c)"),
}
PARITY_CASES = tuple(c for c in CASES if c != "vo")
_built, _streams = {}, {}


def build(name, P):
    """the named case; a stream is generated once per process and shared by the cases on it (frames() keeps what the hooks made)"""
    if name not in _built:
        make, requests, about = CASES[name]
        if make not in _streams:
            _streams[make] = make(P)
            _streams[make].frames()
        _built[name] = Case(name, _streams[make], requests, about)
    return _built[name]


# ------------------------------------------------------------------------------------------------------------- requests
def in_problem_rows(lm, W):
    """rows of a landmarks_ex table that the next solve has in its problem: not dynamic, at least 2 observations, start < W - 2"""
    return (lm[:, 6] == 0) & (lm[:, 2] >= 2) & (lm[:, 1] < W - 2)


def resolve(case, rq, k, maps, window, lm):
    """(stamp, frame index, match points [n][3] or None, p, R) of request rq made after stream frame k; maps[f] = (ids, obs) of the stream
    frames so far, window / lm the pipeline's window and landmarks_ex table after frame k"""
    st, W = case.stream, case.cfg.window_size
    stamp_i = float(window[rq.index, 16])
    kk = max(0, int(np.argmin(np.abs(st.stamps - stamp_i))) - rq.back)
    union = {}
    for f in range(kk, k + 1):
        for fid, o in zip(*maps[f]):
            union.setdefault(int(fid), (float(o[0]), float(o[1])))
    ids = np.array(sorted(union), np.int64)
    xy = np.array([union[i] for i in ids]).reshape(-1, 2)
    inp = in_problem_rows(lm, W)
    usable = set(lm[inp & (lm[:, 1] <= rq.index), 0].astype(np.int64).tolist())       # would be a factor if matched
    if rq.select == "absent":
        ids = ids + ABSENT_ID
        assert ids.min() > st.next_id
    elif rq.select == "first":
        keep = np.nonzero(np.isin(ids, sorted(usable)))[0][len(usable) // 2:len(usable) // 2 + rq.count]
        ids, xy = ids[keep], xy[keep]
    elif rq.select == "not_in_problem":
        table = set(lm[:, 0].astype(np.int64).tolist())
        keep = np.array([i in table and i not in usable for i in ids])
        ids, xy = ids[keep], xy[keep]
    elif rq.select == "ends":
        cap = BC.tracker_capacity(case.cfg)
        u = np.array(sorted(usable))
        a, b = int(u[0]), int(u[-1])
        pad = a + 1 + np.arange(cap - 2)
        assert pad[-1] < b and not set(pad.tolist()) & set(lm[:, 0].astype(np.int64).tolist())
        xy = np.vstack([union[a], np.zeros((cap - 2, 2)), union[b]])
        ids = np.concatenate([[a], pad, [b]])
    mp = None if rq.select == "empty" else np.ascontiguousarray(np.c_[xy, ids.astype(np.float64)])
    p, R = st.scene.pose(float(st.stamps[kk]))
    if rq.yaw_deg:
        a = np.radians(rq.yaw_deg)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        p, R = Rz @ p, Rz @ R
    return (UNKNOWN_STAMP if rq.unknown else stamp_i, FRAME_INDEX, mp, np.ascontiguousarray(p), np.ascontiguousarray(R))


# ------------------------------------------------------------------------------------------------------------- driver
def drive(case, acc, resolved=None, frames=None, skip_requests=False):
    """the case over a pipeline.  acc: make(cfg), push_imu(pipe, t, acc, gyr), process(pipe, ids, obs, depth, stamp), record(pipe) (the
    per-frame record of test_gpu_backend_edges._record: status, window, lm, prior), relo(pipe), set_relo(pipe, stamp, index, mp, p, R),
    close(pipe).  resolved: the arguments of every request as an earlier run returned them (the same request for a second pipeline).
    Returns dict(frames = [record + relo per frame], requests = [dict(after, args, relo = relo() read right after the request, before any
    solve)])"""
    st = case.stream
    pipe = acc["make"](st.cfg)
    maps, out, reqs = {}, [], []
    for k, (stamp, ids, obs, depth, (ti, ai, gi)) in enumerate(st.frames()[:frames]):
        if len(ti):
            acc["push_imu"](pipe, ti, ai, gi)
        acc["process"](pipe, ids, obs, depth, stamp)
        maps[k] = (ids, obs)
        rec = acc["record"](pipe)
        rec["relo"] = acc["relo"](pipe)
        out.append(rec)
        for n, rq in enumerate(case.requests):
            if rq.after != k or skip_requests:
                continue
            args = resolved[n] if resolved is not None else resolve(case, rq, k, maps, rec["window"], rec["lm"])
            acc["set_relo"](pipe, *args)
            reqs.append(dict(after=k, args=args, relo=acc["relo"](pipe)))
    acc["close"](pipe)
    return dict(frames=out, requests=reqs)


def oracle_accessors(matched=False):
    """OraclePipeline through the accessors of drive(); the record carries the oracle's line-search and bound counters as well.  matched:
    the caller has set OVIO_DEVIATIONS = 31 around the run (the prior is then kept as (A, b) itself, backend_cases.prior_quadratic)"""
    import vio_ct

    def record(o):
        pr = o.prior()
        return dict(status=o.status(), window=o.window().copy(), lm=o.landmarks_ex().copy(), prior=None if pr is None else BC.prior_quadratic(pr, matched),
                    line_search=o.line_search_stats(), bounds=o.bound_stats())
    return dict(make=lambda cfg: vio_ct.OraclePipeline(cfg), push_imu=lambda o, t, a, g: o.push_imu(t, a, g),
                process=lambda o, ids, obs, depth, stamp: o.process_obs(ids, obs, BC.oracle_depth(depth), stamp), record=record,
                relo=lambda o: o.relo(), set_relo=lambda o, stamp, index, mp, p, R: o.set_relo_frame(stamp, index, np.zeros((0, 3)) if mp is None else mp, p, R),
                close=lambda o: None)


def run_oracle(case, matched=False):
    return drive(case, oracle_accessors(matched))


def solve_frame(case, n=-1):
    """the stream frame whose solve carries request n (the one after it was made; the frame that ends the initialisation if it was made before)"""
    return max(case.requests[n].after + 1, case.cfg.window_size)


def oracle_formulation_gap(P, name):
    """what the oracle's own two formulations (OVIO_DEVIATIONS = 31 against 0) leave between them on the relocalisation solve of a case:
    dict(relo_pose, relative_t, drift_t (m), relative_q (unit quaternion, up to sign))"""
    import os
    import vio_ct
    case = build(name, P)
    base = run_oracle(case)
    os.environ["OVIO_DEVIATIONS"] = "31"
    try:
        dev = drive(case, oracle_accessors(True), resolved=[r["args"] for r in base["requests"]])
    finally:
        os.environ.pop("OVIO_DEVIATIONS", None)
        vio_ct.oracle().ovio_set_deviations(0)
    a, b = base["frames"][solve_frame(case)]["relo"], dev["frames"][solve_frame(case)]["relo"]
    out = {key: float(np.abs(a[key] - b[key]).max()) for key in ("relative_t", "drift_t")}
    out["relo_pose"] = float(np.abs(a["relo_pose"][:3] - b["relo_pose"][:3]).max())
    out["relative_q"] = float(min(np.abs(a["relative_q"] - b["relative_q"]).max(), np.abs(a["relative_q"] + b["relative_q"]).max()))
    return out


if __name__ == "__main__":
    import vio_ct
    for case in ("single", "no_overlap", "empty", "not_in_problem"):
        print("%-15s" % case, " ".join("%s %.1e" % kv for kv in sorted(oracle_formulation_gap(vio_ct.pkg(), case).items())))
