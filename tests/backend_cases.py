"""Generated feature-map streams that drive the back end (be_ingest -> solve -> be_marg -> be_finish) to its structural edges through
vio_process_obs / OraclePipeline.process_obs: no images, no tracker.

A stream is a body trajectory that may hold still over intervals, a fixed landmark cloud seen through a known extrinsic, a list of frame
stamps (irregular where a case needs it) and an IMU rate.  IMU samples are finite differences of the analytic pose without noise
(excalib_ref.Scene.imu, which CaseScene inherits); per-case hooks rewrite a frame's map (permute, remap ids, drop / re-introduce ids, edit
depth pixels).  CASES names the streams; tests/test_backend_cases_cpu.py shows on the oracle alone that each reaches its branch,
tests/test_gpu_backend_edges.py compares the HIP back end with the oracle on them.

The image is 64 x 64 (the smallest a handle accepts; the back end reads it only for depth look-ups), fx = fy = 32, cx = cy = 32."""
import numpy as np

import excalib_ref as X

WIDTH = HEIGHT = 64
FOCAL = 32.0
INT32_MAX = 2 ** 31 - 1
HASH_MULT = 2654435761       # be_ingest: bucket = (unsigned)id * 2654435761u & (HT - 1)
IMU_SLOT_CAP = 64            # VIO_IMU_SLOT_CAP (csrc/vio_state.h)
PI_CH = 8                    # chunk of the pre-integration loops (csrc/kernels.h)
IMU_COUNTS = (1, 2, 7, 8, 9, 16, 17, 63, 64)

STATUS_KEYS = ("solver_flag", "frame_count", "marginalization_flag", "n_landmarks", "last_track_num", "n_in_problem", "n_residuals",
               "n_var_landmarks", "iterations", "successful_steps")


# ------------------------------------------------------------------------------------------------------------- capacities
def tracker_capacity(cfg):
    """NP of vio_create (vio_get_capacity 'tracks'): the largest feature map a handle takes"""
    ncells = cfg.grid_rows * cfg.grid_cols
    return (cfg.max_cnt + ncells * (cfg.max_cnt // ncells + 2) + 8 + 7) & ~7


def landmark_capacity(cfg):
    """NL of vio_create (vio_get_capacity 'landmarks')"""
    return (max(cfg.max_landmarks, tracker_capacity(cfg)) + 7) & ~7


def lm_hash_size(n_landmarks_cap):
    """HT of be_ingest's id -> slot table for a landmark capacity: the power of two >= max(256, 2 NL)"""
    ht = 256
    while ht < 2 * n_landmarks_cap:
        ht <<= 1
    return ht


def hash_bucket(fid, ht):
    return (((int(fid) & 0xFFFFFFFF) * HASH_MULT) & 0xFFFFFFFF) & (ht - 1)


def case_config(P, **kw):
    d = dict(width=WIDTH, height=HEIGHT, fx=FOCAL, fy=FOCAL, cx=WIDTH / 2.0, cy=HEIGHT / 2.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, max_cnt=40,
             grid_rows=1, grid_cols=1, window_size=4, max_landmarks=200)
    d.update(kw)
    cfg = P.canonical_config(**d)
    for i in range(9):
        cfg.ric[i] = float(X.RIC_TRUE.reshape(-1)[i])
    for i in range(3):
        cfg.tic[i] = float(X.TIC_TRUE[i])
    return cfg


# ------------------------------------------------------------------------------------------------------------- trajectory
def _ramp(x):
    """integral of the quintic smoothstep: 0 for x <= 0, x - 1/2 for x >= 1, C^3 in between"""
    x = np.maximum(x, 0.0)
    return np.where(x < 1.0, x ** 6 - 3.0 * x ** 5 + 2.5 * x ** 4, x - 0.5)


class CaseScene(X.Scene):
    """moves = [(t_start, t_end, speed)]: the path parameter s advances at `speed` inside each interval (blended in and out over `blend`
    seconds) and is EXACTLY constant outside: the rig holds still there, the IMU reads gravity only.  The cloud: `base` landmarks on a 7 x 7
    pixel lattice of the pose at t = 0 (8 px apart, depths 3 .. 9 m, so that no two of them ever share a depth pixel under the small motions
    used here) and 36 `extra` ones on the half-lattice, which only hooks show."""

    def __init__(self, cfg, moves, imu_rate, blend=0.25, amp=0.4, rot=0.05, seed=3, ric=None, tic=None):
        self.cfg, self.ric, self.tic = cfg, (X.RIC_TRUE if ric is None else ric), (X.TIC_TRUE if tic is None else tic)
        self.moves, self.blend, self.amp, self.rot = [tuple(float(v) for v in m) for m in moves], float(blend), float(amp), float(rot)
        self.imu_rate = float(imu_rate)
        rs = np.random.RandomState(seed)
        uv = [(8.0 * (i + 1) + 0.4, 8.0 * (j + 1) + 0.4) for j in range(7) for i in range(7)]
        self.n_base = len(uv)
        uv += [(8.0 * (i + 1) + 4.4, 8.0 * (j + 1) + 4.4) for j in range(6) for i in range(6)]
        uv = np.array(uv)
        z = rs.uniform(3.0, 9.0, len(uv))
        Pc = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * z, (uv[:, 1] - cfg.cy) / cfg.fy * z, z], 1)
        p, R = self.pose(0.0)
        self.L = Pc @ (R @ self.ric).T + (p + R @ self.tic)

    def s(self, t):
        b = self.blend
        return float(sum(v * b * (_ramp((t - a) / b) - _ramp((t - (e - b)) / b)) for a, e, v in self.moves))

    def pose(self, t):
        s, a, r = self.s(t), self.amp, self.rot
        p = a * np.array([np.sin(1.2 * s), np.sin(1.0 * s + 2.0) - np.sin(2.0), 0.5 * (np.sin(1.4 * s + 0.5) - np.sin(0.5))])
        return p, X.rodrigues(r * np.array([np.sin(1.3 * s + 1.9) - np.sin(1.9), np.sin(0.9 * s + 0.7) - np.sin(0.7), np.sin(1.1 * s)]))

    def project(self, t):
        """(x, y, z, u, v) of every landmark in the camera at time t"""
        p, R = self.pose(t)
        Pc = (self.L - (p + R @ self.tic)) @ (R @ self.ric)
        z = Pc[:, 2]
        x, y = Pc[:, 0] / z, Pc[:, 1] / z
        return x, y, z, self.cfg.fx * x + self.cfg.cx, self.cfg.fy * y + self.cfg.cy


class MutableFrame:
    """what a hook edits: lm (landmark index of every observation), ids, obs [n][7] = (x, y, 1, u, v, vx, vy), depth [H][W] u16"""

    def __init__(self, k, stamp, proj, prev):
        self.k, self.stamp, self.proj, self.prev = k, stamp, proj, prev
        self.lm, self.ids, self.obs = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 7))
        self.depth = np.zeros((HEIGHT, WIDTH), np.uint16)

    def pixel(self, j):
        return int(self.proj[4][j]), int(self.proj[3][j])

    def add(self, lms, ids):
        """observations of landmarks lms under ids, with their true depth in the depth image; a landmark whose pixel is taken is left out"""
        x, y, z, u, v = self.proj
        for j, fid in zip(lms, ids):
            r, c = self.pixel(j)
            if not (z[j] > 0.5 and 1 <= u[j] < WIDTH - 1 and 1 <= v[j] < HEIGHT - 1) or self.depth[r, c] != 0:
                continue
            o = np.array([x[j], y[j], 1.0, u[j], v[j], 0.0, 0.0])
            if self.prev is not None and j in self.prev[1]:
                o[5:7] = (o[0:2] - self.prev[1][j]) / (self.stamp - self.prev[0])
            self.depth[r, c] = int(round(z[j] * 1000.0))
            self.lm, self.ids, self.obs = np.append(self.lm, j), np.append(self.ids, fid), np.vstack([self.obs, o])

    def keep(self, mask):
        """drops the observations where mask is False (their depth pixels are cleared)"""
        mask = np.asarray(mask, bool)
        for j in self.lm[~mask]:
            self.depth[self.pixel(j)] = 0
        self.lm, self.ids, self.obs = self.lm[mask], self.ids[mask], self.obs[mask]

    def permute(self, order):
        self.lm, self.ids, self.obs = self.lm[order], self.ids[order], self.obs[order]

    def index(self, j):
        return int(np.nonzero(self.lm == j)[0][0])


class Stream:
    """frames(): [(stamp, ids int32 [n], obs [n][7], depth u16 [H][W], (t, acc, gyr) of the IMU samples to push before the frame)].
    ids_of[j] is the id landmark j is currently published under; a hook that drops a landmark for a frame renews its id (renew), as a
    tracker would, unless the case is about the id coming back."""

    def __init__(self, name, cfg, scene, stamps, hooks=(), about=""):
        self.name, self.cfg, self.scene, self.stamps, self.hooks, self.about = name, cfg, scene, np.asarray(stamps, np.float64), list(hooks), about
        self.ids_of = np.arange(len(scene.L), dtype=np.int64)
        self.next_id = len(scene.L)
        self.notes = {}          # what hooks record for the tests (frame numbers, ids)
        self._frames = None

    def renew(self, lms):
        for j in np.atleast_1d(lms):
            self.ids_of[j] = self.next_id
            self.next_id += 1

    def imu_counts(self):
        """per frame, the samples getIMUInterval hands to processIMU (td = 0): those with prev stamp < t < stamp, plus the first at or
        after the stamp; frame 0 starts at -inf"""
        ts = self.scene.imu(self.stamps[-1] + 1.0)[0]
        out, prev = [], -np.inf
        for t in self.stamps:
            out.append(int(np.count_nonzero((ts > prev) & (ts < t))) + 1)
            prev = t
        return out

    def frames(self):
        if self._frames is not None:
            return self._frames
        sc = self.scene
        ts, acc, gyr = sc.imu(self.stamps[-1] + 1.0)
        out, k0, prev = [], 0, None
        for k, t in enumerate(self.stamps):
            k2 = min(int(np.searchsorted(ts, t + 2.0 / sc.imu_rate, "left")) + 1, len(ts))   # (two samples beyond the stamp: td may grow)
            fr = MutableFrame(k, float(t), sc.project(float(t)), prev)
            base = np.arange(sc.n_base)
            fr.add(base, self.ids_of[base])
            self.renew(np.setdiff1d(base, fr.lm))     # a landmark that left the view comes back under a fresh id, as from a tracker
            for h in self.hooks:
                h(self, fr)
            assert len(fr.ids) <= tracker_capacity(self.cfg) and (len(fr.ids) == 0 or fr.ids.min() >= 0)
            prev = (float(t), {int(j): fr.obs[i, 0:2].copy() for i, j in enumerate(fr.lm)})
            out.append((float(t), fr.ids.astype(np.int32), np.ascontiguousarray(fr.obs), fr.depth, (ts[k0:k2], acc[k0:k2], gyr[k0:k2])))
            k0 = k2
        self._frames = out
        return out


def oracle_depth(depth):
    """the depth image as the oracle (and the reference) must be given it: they index it without clamping, so an observation in row
    `height` reads one row past the image.  One more row, a copy of the last, is what the HIP look-up's clamp reads there."""
    return np.ascontiguousarray(np.vstack([depth, depth[-1:]]))


# ------------------------------------------------------------------------------------------------------------- hooks
def thin_to(n_tracked, frames):
    """on the given frames all but n_tracked landmarks get fresh ids: last_track_num = n_tracked there"""
    def hook(st, fr):
        if fr.k in frames:
            st.renew(fr.lm[n_tracked:])
            fr.ids = st.ids_of[fr.lm].copy()
    return hook


def shuffle_maps(seed):
    def hook(st, fr):
        fr.permute(np.random.RandomState(seed + fr.k).permutation(len(fr.ids)))
    return hook


def show_extras(plan):
    """plan = {frame: [(first extra, count, frames shown)]}: extra landmarks first .. first + count appear under fresh ids on `frame` and stay
    for `frames shown` frames"""
    live = []

    def hook(st, fr):
        for first, count, shown in plan.get(fr.k, ()):
            lms = st.scene.n_base + np.arange(first, first + count)
            st.renew(lms)
            live.append((fr.k + shown, lms))
            st.notes.setdefault("extras", {}).setdefault(fr.k, []).extend(int(i) for i in st.ids_of[lms])
        for until, lms in live:
            if fr.k < until:
                fr.add(lms, st.ids_of[lms])
    return hook


# ------------------------------------------------------------------------------------------------------------- streams
def _stamps(n, rate, t0=1.0):
    return t0 + np.arange(n) / rate + 0.37 / 200.0


def _standstill(name, P, hold, about, W=4, **cfg_kw):
    """2 Hz camera, 50 Hz IMU (25 samples per frame): static initialisation, 3 keyframes, `hold` frames without motion (every one a
    non-keyframe merged into slot W - 1), then W + 3 keyframes"""
    cfg = case_config(P, window_size=W, **cfg_kw)
    rate = 2.0
    n = (W + 1) + 3 + hold + (W + 3) + 1
    stamps = _stamps(n, rate)
    t_go, t_stop = stamps[W], stamps[W + 4]
    t_again = stamps[W + 4 + hold - 1]
    sc = CaseScene(cfg, [(t_go, t_stop, 1.0), (t_again, stamps[-1] + 2.0, 1.0)], 50.0)
    return Stream(name, cfg, sc, stamps, about=about)


def standstill(P):
    return _standstill("standstill", P, 23, "a merged slot that spans more than 10 s: its IMU factor is skipped in the solves and, once the interval "
                       "has slid down to slot 1, in the MARGIN_OLD marginalisation")


def standstill_short(P):
    return _standstill("standstill_short", P, 14, "control: the same stream with the hold cut to 14 frames (longest interval 7 s): every factor kept")


def w10_td(P):
    """window_size 10 with td and the extrinsic estimated: the hold is sampled at 1 Hz (50 samples per frame) to fit 40 frames"""
    W = 10
    cfg = case_config(P, window_size=W, estimate_td=1, estimate_extrinsic=1)
    s1 = _stamps(W + 1 + 3, 2.0)
    hold = s1[-1] + 1.0 * np.arange(1, 13)
    s3 = hold[-1] + 0.5 * np.arange(1, W + 3 + 1)
    stamps = np.concatenate([s1, hold, s3])
    sc = CaseScene(cfg, [(stamps[W], stamps[W + 3] + 0.5, 1.0), (hold[-2], stamps[-1] + 2.0, 1.0)], 50.0)
    return Stream("w10_td", cfg, sc, stamps, about="the standstill branches with the td and extrinsic columns present")


def _imu_count_stream(name, P, counts_after_init, thin_frames, about):
    """200 Hz IMU, a slow drift (parallax far below the keyframe threshold, so a frame is a keyframe exactly when its map is thinned to 19
    tracked features): frame k + 1 lies counts[k] - 1 IMU samples after frame k, at a phase inside the sample interval that keeps stamps
    distinct when the count is 1"""
    cfg = case_config(P)
    rate, W = 200.0, cfg.window_size
    m, ph, stamps = 200, 0.2, []
    for c in [21] * (W + 1) + list(counts_after_init):
        ph = ph + 0.2 if c == 1 else 0.2
        m += c - 1
        stamps.append((m + ph) / rate)
    sc = CaseScene(cfg, [(stamps[W], stamps[-1] + 2.0, 0.05)], rate)
    return Stream(name, cfg, sc, stamps, hooks=[thin_to(19, set(thin_frames))], about=about)


def imu_counts(P):
    W = 4
    counts, thin = [21, 21], []
    for c in IMU_COUNTS:      # each count on a non-keyframe, then on a keyframe
        counts += [c, c]
        thin.append(W + 1 + len(counts) - 1)
    counts += [21, 21]
    return _imu_count_stream("imu_counts", P, counts, thin, "PI_CH chunk edges in the new-frame propagation and in the MARGIN_SECOND_NEW merge; "
                             "the 64-sample slot buffer exactly full")


def imu_65(P):
    st = _imu_count_stream("imu_65", P, [21, 21, 21, 65, 21, 21, 21, 21, 21, 21], [], "one non-keyframe with 65 samples: overflow bit 2")
    st.notes["overflow_frame"], st.notes["overflow_bit"] = 4 + 1 + 3, 2
    return st


def _moving(P, n, rate=5.0, imu_rate=100.0, pauses=(), speed=1.0, **cfg_kw):
    cfg = case_config(P, **cfg_kw)
    W = cfg.window_size
    stamps = _stamps(n, rate)
    moves, a = [], stamps[W]
    for p0, p1 in pauses:
        moves.append((a, stamps[p0], speed))
        a = stamps[p1]
    moves.append((a, stamps[-1] + 2.0, speed))
    return cfg, CaseScene(cfg, moves, imu_rate), stamps


def hash_chain(P, **cfg_kw):
    """24 landmarks under ids base + j HT (one bucket, and base is chosen so that the chain starts three buckets before the end of the table
    and wraps), one under INT32_MAX - 1, one under 0, the rest ordinary; every map in another order"""
    cfg, sc, stamps = _moving(P, 22, **cfg_kw)
    ht = lm_hash_size(landmark_capacity(cfg))
    base = next(b for b in range(1, 1 << 20) if hash_bucket(b, ht) == ht - 3)
    st = Stream("hash_chain", cfg, sc, stamps, hooks=[shuffle_maps(11)], about="long probe chains, unsorted maps")
    st.ids_of[:24] = base + ht * np.arange(24)
    st.ids_of[24] = INT32_MAX - 1
    st.ids_of[25:sc.n_base] = 100000 + np.arange(sc.n_base - 25)
    st.ids_of[25] = 0
    st.next_id = 200000
    st.notes.update(ht=ht, chain=[int(i) for i in st.ids_of[:24]])
    return st


def reappear(P):
    """landmarks 0 .. 7 leave the map on frames 9 and 10 and return under their old ids: the back end, like the reference, files the returning
    observation under the next frame of the landmark's track, not the frame it was made in, the solver drives the depth of such a landmark
    negative sooner or later, removeFailures drops it, and its id, still in the map, is appended again at the END of the list.  Landmarks
    40 .. 45 lose their depth pixels from frame 9 on and have their displacement since frame 8 mirrored (a point that moves against its
    parallax): movingConsistencyCheck marks them dynamic and they stay in the list, excluded from the solves, while the map keeps their ids"""
    cfg, sc, stamps = _moving(P, 24)
    ref = {}

    def hook(st, fr):
        if fr.k in (9, 10):
            fr.keep(fr.lm >= 8)
        if fr.k == 8:
            ref.update({int(j): fr.obs[fr.index(j), 0:2].copy() for j in range(40, 46) if j in fr.lm})
        if fr.k >= 9:
            for j in ref:
                if j in fr.lm:
                    i = fr.index(j)
                    fr.obs[i, 0:2] = ref[j] - 3.0 * (fr.obs[i, 0:2] - ref[j])
                    fr.depth[fr.pixel(j)] = 0
    st = Stream("reappear", cfg, sc, stamps, hooks=[hook], about="re-appended landmarks, a list not sorted by id")
    st.notes.update(vanish=list(range(0, 8)), culled=list(range(40, 46)))
    return st


def thin(P, **cfg_kw):
    """frame 9: 19 tracked (a keyframe by the first rule, where the parallax rule says no); frame 10: 20 tracked (the parallax rule decides:
    no keyframe); frame 12: every id renewed, so that on frame 13 no landmark spans frames fc - 2 and fc - 1
    (pnum == 0 with every feature tracked); frame 15: a single observation"""
    cfg, sc, stamps = _moving(P, 22, **cfg_kw)

    def hook(st, fr):
        if fr.k == 15:
            st.renew(fr.lm[1:])
            fr.keep(np.arange(len(fr.lm)) < 1)
    st = Stream("thin", cfg, sc, stamps, hooks=[thin_to(19, {9}), thin_to(20, {10}), thin_to(0, {12}), hook], about="the three keyframe rules")
    st.notes.update(f19=9, f20=10, f_pnum0=13, f_single=15)
    return st


# landmark -> (u, v) override; the three that are clamped to the last column lie in different lattice rows, so that no two share a pixel
EDGE_PIXELS = {10: (-0.5, None), 18: (float(WIDTH), None), 12: (None, float(HEIGHT)), 27: (WIDTH + 5.0, None)}


def depth_edges(P, **cfg_kw):
    """from frame 7 on: landmark 3 without depth on every frame (depth-less triangulation needs every observation without depth: it gets a
    fresh id first), landmark 5 at depth_min mm - 1 (skipped for good), landmark 6 at depth_min mm on frame 9 only, landmark 8 just above
    depth_max on frame 9 only; pixel coordinates of landmarks 10, 18, 12 and 27 moved to -0.5, width, height and width + 5 on frames 8 .. 10, with
    their depth at the pixel the clamp reads (and at the pixel the oracle's unclamped index reads)"""
    cfg, sc, stamps = _moving(P, 20, **cfg_kw)
    dmin, dmax = int(round(cfg.depth_min * 1000)), int(round(cfg.depth_max * 1000))

    def hook(st, fr):
        if fr.k == 7:
            st.renew([3])
            fr.ids = st.ids_of[fr.lm].copy()
        if fr.k >= 7:
            if 3 in fr.lm:
                fr.depth[fr.pixel(3)] = 0
            if 5 in fr.lm:
                fr.depth[fr.pixel(5)] = dmin - 1
        if fr.k == 9:
            if 6 in fr.lm:
                fr.depth[fr.pixel(6)] = dmin
            if 8 in fr.lm:
                fr.depth[fr.pixel(8)] = dmax + 1
        if 8 <= fr.k <= 10:
            for j, (u, v) in EDGE_PIXELS.items():
                if j not in fr.lm:
                    continue
                i = fr.index(j)
                r, c = fr.pixel(j)
                mm = fr.depth[r, c]
                fr.depth[r, c] = 0
                if u is not None:
                    fr.obs[i, 3] = u
                    fr.depth[r, min(max(int(u), 0), WIDTH - 1)] = mm     # the clamped look-up
                    if int(u) >= WIDTH:
                        fr.depth[r + 1, int(u) - WIDTH] = mm             # row * width + u without the clamp
                else:
                    fr.obs[i, 4] = v
                    fr.depth[HEIGHT - 1, c] = mm                         # (oracle_depth repeats the last row)
    st = Stream("depth_edges", cfg, sc, stamps, hooks=[hook], about="the depth skip rule, the clamp of the look-up, depth-less triangulation")
    st.notes.update(skipped_lm=5, depthless_lm=3)
    return st


def short_tracks(P):
    """extras seen on frames 8 / 8 - 9 / 8 - 10 only: when frame 8 is frame 0 of the window and leaves it they have 1, 2 and 3 observations;
    extras that first appear on frames 19 and 20, non-keyframes inside a pause: they start in frame W and are moved by removeFront"""
    cfg, sc, stamps = _moving(P, 28, pauses=[(15, 23)], speed=2.5)   # (fast enough that every moving frame is a keyframe)
    st = Stream("short_tracks", cfg, sc, stamps, hooks=[show_extras({8: [(0, 3, 1), (3, 3, 2), (6, 3, 3)], 19: [(12, 4, 3)], 20: [(18, 4, 3)]})],
                about="removeBackShiftDepth with fewer than 2 observations left, removeFront of a landmark that starts in frame W")
    st.notes.update(f_short=8, f_front=(19, 20))
    return st


TABLE_FULL_PLAN = {8: [(0, 36, 1)], 9: [(0, 11, 1)], 10: [(12, 1, 1)]}


def table_full(P):
    """max_landmarks at the handle's minimum (the tracker capacity, 96): fresh ids on frames 8 and 9 until the table holds exactly 96 when
    frame 9 is ingested, then more new ids on frame 10 than the table has room for"""
    cfg, sc, stamps = _moving(P, 20, max_landmarks=1, speed=2.5)     # (every moving frame a keyframe: no frame is dropped from the window)
    st = Stream("table_full", cfg, sc, stamps, hooks=[show_extras(TABLE_FULL_PLAN)], about="the landmark table exactly full, then overflow bit 1")
    st.notes.update(overflow_frame=10, overflow_bit=1, full_frame=9)
    return st


def w20_moving(P):
    """window_size 20, the largest: n = 6 W + 16 = 136 prior parameters, beyond the 128 the LDS-resident eigen-solver of the literal marginalisation
    covers.  W + 14 moving frames; not in CASES (the per-case suites run windows of 4 and 10), generated once per process like them"""
    if "w20_moving" not in _built:
        W = 20
        cfg, sc, stamps = _moving(P, W + 14, window_size=W, speed=2.5)
        _built["w20_moving"] = Stream("w20_moving", cfg, sc, stamps, about="a 20-frame window: the HBM branch of the literal prior")
        _built["w20_moving"].frames()
    return _built["w20_moving"]


CASES = dict(standstill=standstill, standstill_short=standstill_short, imu_counts=imu_counts, imu_65=imu_65, hash_chain=hash_chain,
             reappear=reappear, thin=thin, depth_edges=depth_edges, short_tracks=short_tracks, table_full=table_full, w10_td=w10_td)
PARITY_CASES = tuple(c for c in CASES if c not in ("imu_65", "table_full"))
_built = {}


def anchored(rec):
    """landmarks of a frame's table that start in frame 0 with at least two observations: what the NEXT frame's MARGIN_OLD marginalisation
    eliminates (in_problem), if they are not dynamic"""
    lm = rec["lm"]
    return int(np.count_nonzero((lm[:, 1] == 0) & (lm[:, 2] >= 2) & (lm[:, 6] == 0))) if len(lm) else 0


def build(name, P):
    """the named stream, generated once per process"""
    if name not in _built:
        _built[name] = CASES[name](P)
        _built[name].frames()
    return _built[name]


# ------------------------------------------------------------------------------------------------------------- VO streams
# use_imu = 0 (no IMU samples pushed), fix_depth = 1 and depth_max = 10 (with free depths and no IMU the scale is a gauge freedom of the window:
# test_gpu_vo.test_vo_pipeline_matches_oracle), window 4.  Every frame after the initialisation starts from FeatureManager::initFramePoseByPnP.
def vo_config(P, **kw):
    cfg = case_config(P, fix_depth=1, depth_max=10.0, **kw)
    cfg.use_imu = 0
    return cfg


class RingScene(CaseScene):
    """landmarks on a ring around the rig (160 of them 3 .. 6 m away, heights within the 90 degree field of view: about 40 visible); the body
    yaws `yaw_deg` per frame about its z axis (the camera pans) with a small translation, from frame `hold` on: over the initialisation window
    it stands still at the identity, so that the VO world frame is the frame the truth is written in and the first solve, which starts from
    copies of the first pose, starts at its optimum (a first solve that starts 16 degrees off is decided by round-off: the oracle's own two
    formulations end 1e-4 m apart on it)."""

    def __init__(self, cfg, stamps, yaw_deg, hold, seed=5):
        self.cfg, self.ric, self.tic = cfg, X.RIC_TRUE, X.TIC_TRUE
        self.t0, self.dt, self.yaw, self.hold = float(stamps[0]), float(stamps[1] - stamps[0]), np.radians(yaw_deg), hold
        self.imu_rate = 100.0
        rs = np.random.RandomState(seed)
        n = 160
        az = 2 * np.pi * (np.arange(n) + rs.uniform(-0.3, 0.3, n)) / n
        rad = rs.uniform(3.0, 6.0, n)
        self.L = np.stack([rad * np.cos(az), rad * np.sin(az), rad * rs.uniform(-0.6, 0.6, n)], 1)
        self.n_base = n

    def pose(self, t):
        k = max((t - self.t0) / self.dt - self.hold, 0.0)
        a = self.yaw * k
        return 0.05 * np.array([np.sin(0.3 * k), 1 - np.cos(0.2 * k), 0.5 * np.sin(0.25 * k)]), X.rodrigues([0.0, 0.0, a])

    def imu(self, t_end):
        return np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))


def vo_half_turn(P):
    """the initialisation window at rest, then 56 frames at -4.08 degrees of yaw each (224 degrees; the rate puts the crossing midway between
    two frames): cfg.ric alone is a 120 degree rotation, and the angle of the solvePnP start rotation
    (Rs[fc - 1] ric)^T climbs to pi and comes down again with the axis on the other side: the matrix -> vector branch near pi, then a
    start vector whose hemisphere flipped against the frame before"""
    cfg = vo_config(P)
    stamps = _stamps(cfg.window_size + 56, 5.0)
    st = Stream("vo_half_turn", cfg, RingScene(cfg, stamps, -4.08, cfg.window_size), stamps, about="the solvePnP start rotation passes through pi")
    return st


def vo_few_pairs(P):
    """all but 5, 4, 3 and 0 landmarks get fresh ids on frames 8, 12, 16 and 20: a landmark that is new in a frame has no depth when
    initFramePoseByPnP runs, so these are the pair counts there; 3 and 0 are below cv::solvePnP's minimum and the copied pose stays"""
    cfg, sc, stamps = _moving(P, 24, fix_depth=1, depth_max=10.0)
    cfg.use_imu = 0
    plan = {8: 5, 12: 4, 16: 3, 20: 0}
    st = Stream("vo_few_pairs", cfg, sc, stamps, hooks=[thin_to(n, {k}) for k, n in plan.items()], about="5, 4, 3 and 0 pairs for solvePnP")
    st.notes["pairs"] = plan
    return st


def vo_depthless(P):
    """frame 8: every second landmark of the map comes back under a fresh id, and on frames 8 .. 10 its depth pixel is zero: it is in the list
    without a depth (lm_depth <= 0) and must stay out of the pair list until triangulateWithDepth gives it one from frame 11's pixel"""
    cfg, sc, stamps = _moving(P, 18, fix_depth=1, depth_max=10.0)
    cfg.use_imu = 0
    st = Stream("vo_depthless", cfg, sc, stamps, about="landmarks without a depth stay out of the solvePnP pairs")

    def hook(st, fr):
        half = fr.lm[1::2]
        if fr.k == 8:
            st.renew(half)
            fr.ids = st.ids_of[fr.lm].copy()
            st.notes["with_depth"] = len(fr.lm) - len(half)
        if 8 <= fr.k <= 10:
            for j in half:
                fr.depth[fr.pixel(j)] = 0
    st.hooks.append(hook)
    st.notes["frames"] = (8, 9, 10)
    return st


def _vo_rest(name, P, identity, about):
    """identity = False: the rig stands over the initialisation window, moves for four frames and stops; identity = True: ric = I, tic = 0
    and the rig never moves, so that Rs stays within rounding of I, the matrix -> vector map returns exactly 0 and tvec is 0 within rounding"""
    cfg = vo_config(P)
    W = cfg.window_size
    stamps = _stamps(W + 12, 5.0)
    ric, tic = (np.eye(3), np.zeros(3)) if identity else (None, None)
    if identity:
        for i in range(9):
            cfg.ric[i] = float(np.eye(3).reshape(-1)[i])
        for i in range(3):
            cfg.tic[i] = 0.0
    moves = [] if identity else [(stamps[W], stamps[W + 4], 1.0)]
    return Stream(name, cfg, CaseScene(cfg, moves, 100.0, ric=ric, tic=tic), stamps, about=about)


def vo_moving_start(P):
    """the rig moves 0.4 m through the initialisation window and on: the first VO solve starts from copies of the first pose, far from its
    optimum (cost 403 over 196 residuals), and has to find the window by itself.  Not one of VO_CASES: landmark 48 fails the consistency test of
    triangulateWithDepth under the copied poses and enters that solve free, with depth -1 and, the poses being identical, no baseline: its
    first step is a rounding residue divided by the damping, so only the first iteration's poses can be compared"""
    cfg = vo_config(P)
    W = cfg.window_size
    stamps = _stamps(W + 8, 5.0)
    return Stream("vo_moving_start", cfg, CaseScene(cfg, [(stamps[0] - 0.3, stamps[W + 2], 1.0)], 100.0), stamps,
                  about="a first VO solve that starts far from its optimum")


def vo_standstill(P):
    return _vo_rest("vo_standstill", P, False, "the rig at rest after the initialisation: solvePnP starts at its optimum")


def vo_identity_extrinsic(P):
    return _vo_rest("vo_identity_extrinsic", P, True, "ric = I, tic = 0, no motion: the first solvePnP start vector is exactly zero")


VO_CASES = dict(vo_half_turn=vo_half_turn, vo_few_pairs=vo_few_pairs, vo_depthless=vo_depthless, vo_standstill=vo_standstill,
                vo_identity_extrinsic=vo_identity_extrinsic)


def build_vo(name, P):
    if name not in _built:
        _built[name] = VO_CASES[name](P)
        _built[name].frames()
    return _built[name]


def run_oracle_vo(st):
    """the oracle over a VO stream (no IMU pushed): per frame dict(rc, status, window, pnp = (called, pairs, start rvec, start tvec))"""
    import vio_ct
    o = vio_ct.OraclePipeline(st.cfg)
    out = []
    for stamp, ids, obs, depth, _ in st.frames():
        rc = o.process_obs(ids, obs, oracle_depth(depth), stamp)
        out.append(dict(rc=rc, status=o.status(), window=o.window().copy(), pnp=o.pnp_info()))
    return out


# ------------------------------------------------------------------------------------------------------------- drivers
def long_interval_slot(window, W, limit=10.0):
    """the highest window slot j in 1 .. W - 1 whose interval Headers[j] - Headers[j - 1] exceeds `limit` seconds, 0 if none (after a slide
    slot W repeats slot W - 1's stamp, so the interval the next solve sees in slot W is not in the table yet)"""
    h = window[:, 16]
    return max([j for j in range(1, W) if h[j] - h[j - 1] > limit], default=0)


def prior_quadratic(pr, matched):
    """(J^T J, J^T r, present) of a prior() result; the matched-formulation oracle keeps (A, b) = (J^T J, J^T r) themselves"""
    J, r, _, pres = pr
    return (J.copy(), r.copy(), pres.copy()) if matched else (J.T @ J, J.T @ r, pres.copy())


def run_oracle(st, matched=False, frames=None):
    """the oracle over the stream: per frame dict(rc, status, window, lm = landmarks_ex, prior = (JtJ, Jtr, present) or None).  matched: the
    caller has set OVIO_DEVIATIONS = 31 around this call"""
    import vio_ct
    o = vio_ct.OraclePipeline(st.cfg)
    out = []
    for stamp, ids, obs, depth, (ti, ai, gi) in st.frames()[:frames]:
        if len(ti):
            o.push_imu(ti, ai, gi)
        rc = o.process_obs(ids, obs, oracle_depth(depth), stamp)
        pr = o.prior()
        out.append(dict(rc=rc, status=o.status(), window=o.window().copy(), lm=o.landmarks_ex().copy(),
                        prior=None if pr is None else prior_quadratic(pr, matched)))
    return out


def oracle_formulation_gap(P, name):
    """what the oracle's own two formulations (OVIO_DEVIATIONS = 31 against 0) leave between them on a stream: (frames before the first
    differing decision or all, worst |dP| over those frames); recorded in DESIGN.md beside the HIP figures"""
    import os
    import vio_ct
    st = build(name, P)
    base = run_oracle(st)
    os.environ["OVIO_DEVIATIONS"] = "31"
    try:
        dev = run_oracle(st, matched=True)
    finally:
        os.environ.pop("OVIO_DEVIATIONS", None)
        vio_ct.oracle().ovio_set_deviations(0)
    n = next((k for k, (a, b) in enumerate(zip(base, dev)) if any(int(a["status"][q]) != int(b["status"][q]) for q in STATUS_KEYS)), len(base))
    return n, len(base), max(float(np.abs(a["window"][:, :3] - b["window"][:, :3]).max()) for a, b in zip(base[:max(n, 1)], dev[:max(n, 1)]))


if __name__ == "__main__":
    import vio_ct
    for case in CASES:
        print("%-17s equal decisions on %2d of %2d frames, max |dP| there %.1e m" % ((case,) + oracle_formulation_gap(vio_ct.pkg(), case)))
