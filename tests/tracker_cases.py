"""Generated grey-image streams that drive the tracker bookkeeping (fe_select / fe_fast / fe_add in csrc/fe_kernels.hip, Tracker::readImage in
oracle/frontend.cpp) into the branches rendered scenes never take.  Plain numpy: Gaussian blobs on a flat background, one noise frame, fixed
seeds.  test_tracker_cases_cpu.py proves on the oracle alone that every case reaches the branch it is named for; test_gpu_tracker_edges.py
compares the kernels with the oracle on the same streams, bit for bit.

A blob narrower than min_dist whose neighbours are further than 2 * min_dist away gives exactly one FAST survivor (its peak pixel) and one
track; identical blobs give exactly equal FAST responses.  The camera has no distortion, so the tracker's float operations are the only
arithmetic between the image and the compared state."""
import numpy as np

import vio_ct

SKIP, TRACK, PUBLISH = 0, 1, 2
W0, H0 = 256, 192
BG, AMP, FWHM = 40.0, 150.0, 3.5
T0, DT = 1.0, 0.1


def blobs(W, H, centres, amps=None, fwhm=FWHM, bg=BG):
    """uint8 image: bg + sum_k amps[k] * exp(-|p - c_k|^2 / (2 sigma^2)), rounded; centres float (x, y), each blob drawn on its 17 x 17 patch"""
    img = np.full((H, W), bg, np.float64)
    s2 = 2.0 * (fwhm / 2.3548200450309493) ** 2
    centres = np.asarray(centres, np.float64).reshape(-1, 2)
    amps = np.full(len(centres), AMP) if amps is None else np.asarray(amps, np.float64)
    for (cx, cy), a in zip(centres, amps):
        x0, x1 = max(int(np.floor(cx)) - 8, 0), min(int(np.floor(cx)) + 9, W)
        y0, y1 = max(int(np.floor(cy)) - 8, 0), min(int(np.floor(cy)) + 9, H)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / s2)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def lattice(W, H, step, x0=10, y0=10, xm=8, ym=8, stepy=None):
    """centres from (x0, y0) to (W - xm, H - ym) every `step` px, row-major"""
    xs, ys = np.arange(x0, W - xm + 1, step), np.arange(y0, H - ym + 1, stepy or step)
    return np.array([(x, y) for y in ys for x in xs], np.float64)


def flat(W, H, v=BG):
    return np.full((H, W), int(v), np.uint8)


def noise(W, H, seed):
    """uniform noise: thousands of FAST survivors (4843 at 256 x 192, seed 9)"""
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


class Case:
    def __init__(self, name, cfg, frames, modes=None, fisheye=None, fast_cap=0):
        self.name, self.cfg, self.frames = name, cfg, [np.ascontiguousarray(f, np.uint8) for f in frames]
        self.modes = list(modes) if modes is not None else [PUBLISH] * len(frames)
        assert len(self.modes) == len(self.frames) and 4 <= len(self.frames) <= 12
        self.stamps = [T0 + DT * k for k in range(len(frames))]
        self.fisheye = None if fisheye is None else np.ascontiguousarray(fisheye, np.uint8)
        self.fast_cap = fast_cap     # what the oracle is told to keep per cell: VIO_FAST_CAP where the case overflows the kernel's buffer


def config(P, W=W0, H=H0, rows=1, cols=1, max_cnt=150, min_dist=4, **kw):
    """no distortion, principal point in the middle, everything else as the default configuration"""
    d = dict(width=W, height=H, grid_rows=rows, grid_cols=cols, max_cnt=max_cnt, min_dist=min_dist, fx=200.0, fy=200.0, cx=W / 2.0, cy=H / 2.0,
             k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    d.update(kw)
    return P.default_config(**d)


def _moving(W, H, centres, n, shift=(0.0, 0.0), amps=None, zoom=1.0):
    """n frames of the same blobs: frame f shows them shifted by f * shift, or scaled by zoom^f about the image centre"""
    c = np.asarray(centres, np.float64)
    mid = np.array([W / 2.0, H / 2.0])
    return [blobs(W, H, (c - mid) * zoom ** f + mid + f * np.asarray(shift, np.float64), amps) for f in range(n)]


def _amps(n, seed, levels=4):
    """amplitudes 100, 125, 150, 175 in random order: the top-k scan replaces slots, and every time the weakest level runs out the newcomer
    ties with the new minimum"""
    return 100.0 + 25.0 * (np.random.default_rng(seed).permutation(n) % levels)


def _two_layers(W, H, n_frames, speeds, late=0, step=(24, 12), gap=12, a_rows=None):
    """layer A: static lattice; layer B: the same lattice `gap` px to the left, row r moving right by speeds[r % len(speeds)] px per frame, so
    that B's blobs close in on A's from a row-dependent frame on.  late: B is absent from the first `late` frames (then A's tracks are older
    than B's).  a_rows: layer A keeps only its first a_rows rows (B keeps all)"""
    A = lattice(W, H, step[0], x0=10 + gap, y0=10, stepy=step[1])
    rows = ((A[:, 1] - 10) // step[1]).astype(int)
    v = np.asarray(speeds, np.float64)[rows % len(speeds)]
    out = []
    for f in range(n_frames):
        B = A + np.stack([-gap + v * max(f - late, 0), np.zeros(len(A))], 1)
        Af = A if a_rows is None else A[rows < a_rows]
        out.append(blobs(W, H, np.concatenate([Af, B]) if f >= late else Af))
    return out


def build(name, P):
    L8, L20 = lattice(W0, H0, 8), lattice(W0, H0, 20)
    if name == "serial_topk":            # 660 identical blobs, one cell, K = 152: nf > K > 64 (serial replay of the scan, all responses tied)
        return Case(name, config(P), _moving(W0, H0, L8, 4))
    if name == "serial_topk_amps":       # the same with four amplitude levels: the serial scan replaces slots
        return Case(name, config(P), _moving(W0, H0, L8, 4, amps=_amps(len(L8), 3)))
    if name == "serial_topk_2cells":     # 1 x 2 grid, K = 77 per cell
        return Case(name, config(P, cols=2), _moving(W0, H0, L8, 4))
    if name == "wave_topk_ties":         # max_cnt 60, K = 62 <= 64: the wavefront scan, all responses tied
        return Case(name, config(P, max_cnt=60), _moving(W0, H0, L8, 4))
    if name == "wave_topk_amps":         # the wavefront scan with replacements, among them candidates that TIE with the current minimum
        return Case(name, config(P, max_cnt=60), _moving(W0, H0, L8, 4, amps=_amps(len(L8), 4)))
    if name == "serial_addpoints":       # 108 blobs, K = 152: 64 < nf <= K (one-by-one addPoints)
        return Case(name, config(P), _moving(W0, H0, L20, 4, shift=(0.3, 0.2)))
    if name == "serial_addpoints_conflicts":   # min_dist 12 and a second blob 9 px right of every third one: the one-by-one walk rejects
        extra = L20[::3] + np.array([9.0, 0.0])
        return Case(name, config(P, min_dist=12), _moving(W0, H0, np.concatenate([L20, extra]), 4))
    if name == "mask_blocks":            # isolated blobs appearing in steps: setMask sees n = 0, 1, 63, 64, 65, 128, 129, 216 (12 px lattice, 300)
        c = lattice(W0, H0, 12, x0=14, y0=12)
        rng = np.random.default_rng(7)
        c = c[rng.permutation(len(c))]
        counts = [1, 63, 64, 65, 128, 129, 216, 216, 216]
        return Case(name, config(P, max_cnt=400), [blobs(W0, H0, c[:k] + f * np.array([1.0, 0.0])) for f, k in enumerate(counts)])
    if name == "mask_collide_equal":     # both layers detected on frame 0 (equal track counts), B closes in on A row after row
        return Case(name, config(P, max_cnt=400, min_dist=10), _two_layers(W0, H0, 8, (1.0, 1.5, 2.0, 0.5, 2.5)))
    if name == "mask_collide_mixed":     # B appears three frames after A (on the frame the cell detects again), and A is only 4 rows of 10: 40 old tracks sort before the fresh ones, so
        # an old blob and the fresh one that runs into it sit 40 places apart -- across a part, the word and the block boundary
        return Case(name, config(P, max_cnt=400, min_dist=10), _two_layers(W0, H0, 8, (0.5, 1.0, 2.0, 2.5, 1.5), late=3, a_rows=4))
    if name == "modes":                  # PUBLISH / TRACK / TRACK / PUBLISH / SKIP / PUBLISH while the layers crowd: a PUBLISH frame starts with
        fr = _two_layers(W0, H0, 7, (1.5, 2.0, 2.5))   # more than max_cnt tracks, many closer than min_dist
        return Case(name, config(P, max_cnt=200, min_dist=10), fr, modes=[PUBLISH, TRACK, TRACK, PUBLISH, SKIP, PUBLISH, PUBLISH])
    if name == "ransac_7_8":             # 7 blobs, then 8, then 9: rejectWithF skipped at n = 7, run at n = 8
        c = np.array([(40, 40), (200, 50), (120, 96), (60, 150), (210, 160), (150, 30), (30, 100), (180, 110), (100, 160)], np.float64)
        counts = [7, 8, 9, 9, 9]
        return Case(name, config(P), [blobs(W0, H0, c[:k] + f * np.array([0.7, 0.3])) for f, k in enumerate(counts)])
    if name == "all_lost":               # blobs, flat, flat (every track dies on the second flat frame: n = 0), blobs, blobs
        b = blobs(W0, H0, L20)
        return Case(name, config(P), [b, flat(W0, H0), flat(W0, H0), b, b, b])
    if name == "flat_first":             # no corner anywhere on the first frames: the cells go textureless, come back, then detect
        b = blobs(W0, H0, L20)
        return Case(name, config(P, rows=2, cols=2), [flat(W0, H0), flat(W0, H0), flat(W0, H0), b, b, b])
    if name == "unstable":               # every other blob vanishes; two frames later (its track just died as an unstable point) a new blob
        a = L20                          # appears 2 px beside the old place: inside the unstable disk, it must not be added
        keep = a[1::2]
        new = a[::2] + np.array([2.0, 1.0])
        lone = np.array([[20.0, 20.0]])   # a fresh blob on frame 1 keeps the cell from going textureless before the frame that matters
        return Case(name, config(P), [blobs(W0, H0, a), blobs(W0, H0, np.concatenate([keep, lone])), blobs(W0, H0, np.concatenate([keep, lone, new])),
                                      blobs(W0, H0, np.concatenate([keep, lone, new])), blobs(W0, H0, np.concatenate([keep, lone, new]))])
    if name == "exits":                  # the lattice grows about the image centre by 1.7 % per frame: tracks leave through all four borders
        return Case(name, config(P, rows=2, cols=2), _moving(W0, H0, lattice(W0, H0, 12, x0=9, y0=6, xm=6, ym=6), 12, zoom=1.017))
    if name == "grid_remainder":         # 255 x 191, 4 x 4 grid: grid_w 63, grid_h 47; blobs drift (+1, +1) into x in [252, 253.5), y in [188, 189.5)
        W, H = 255, 191
        c = np.concatenate([lattice(W, H, 20, x0=12, y0=12, xm=30, ym=30),
                            [(x, y) for y in range(20, 170, 30) for x in (248.0, 249.5, 251.0)],     # right band
                            [(x, y) for x in range(20, 230, 30) for y in (184.0, 185.5, 187.0)],     # bottom band
                            [(250.0, 186.0), (251.0, 187.0)]])                                       # the band's corner
        return Case(name, config(P, W=W, H=H, rows=4, cols=4), _moving(W, H, c, 6, shift=(1.0, 1.0)))
    if name == "grid_remainder_decides":   # the same size with max_cnt 16: grids_threshold 1, so ONE track decides whether a cell detects.  The only
        # track of cells 3, 12 and 15 drifts into the band (frames 2 and 3: x 252, 253 / y 188, 189) while a second blob appears in the cell: counted
        # in its own cell (the decrement) the cell is full and the blob is not detected until the track has left (frame 4); counted anywhere else
        # the cell would be in deficit and add the blob two frames early
        W, H = 255, 191
        first = np.array([(249.0, 20.0), (20.0, 185.0), (249.0, 185.0)])
        second = np.array([(205.0, 28.0), (30.0, 160.0), (215.0, 160.0)])
        return Case(name, config(P, W=W, H=H, rows=4, cols=4, max_cnt=16),
                    [blobs(W, H, (first if f < 3 else np.concatenate([first, second])) + f * np.array([1.0, 1.0])) for f in range(8)])
    if name == "near_cap":               # one cell, min_dist 3, max_cnt 400: 300 tracks survive setMask and the cell is still in deficit
        c = lattice(W0, H0, 12, x0=14, y0=12)
        more = c[::4] + np.array([6.0, 6.0])    # new blobs between the old ones from frame 2 on
        f0 = blobs(W0, H0, c)
        f2 = blobs(W0, H0, np.concatenate([c, more]))
        return Case(name, config(P, max_cnt=400, min_dist=3), [f0, f0, f2, f2])
    if name == "fast_overflow":          # a noise frame with more FAST survivors than the kernel's candidate buffer, between blob frames
        b = blobs(W0, H0, L20)
        b1 = blobs(W0, H0, np.concatenate([L20, [[20.0, 20.0]]]))   # a fresh blob: the cell stays textured for the noise frame
        return Case(name, config(P), [b, b1, noise(W0, H0, 9), b1, b1], fast_cap=1024)
    if name.startswith("fisheye_grey"):  # mask 0 | 128 | 255 in vertical thirds (boundaries x = 85, 170) across a dense lattice drifting left
        m = np.full((H0, W0), 255, np.uint8)
        m[:, :85] = 0
        m[:, 85:170] = 128
        m[60:130, 190:230] = 128         # a grey island inside the white third
        kind = name[len("fisheye_grey_"):]
        cfg = config(P, max_cnt=60) if kind == "wave" else config(P)
        c = L20 if kind == "addpoints" else L8
        return Case(name, cfg, _moving(W0, H0, c, 5, shift=(-1.5, 0.0)), fisheye=m)
    raise KeyError(name)


# The issue's `saturated` case is not a stream of its own: every serial_topk* / wave_topk_* stream is saturated (n >= max_cnt, n_max_cnt <= 0, no
# detection at all) from its second frame on, and test_tracker_cases_cpu.py asserts it there.
NAMES = ("serial_topk", "serial_topk_amps", "serial_topk_2cells", "wave_topk_ties", "wave_topk_amps", "serial_addpoints",
         "serial_addpoints_conflicts", "mask_blocks", "mask_collide_equal", "mask_collide_mixed", "modes", "ransac_7_8", "all_lost", "flat_first",
         "unstable", "exits", "grid_remainder", "grid_remainder_decides", "near_cap", "fast_overflow", "fisheye_grey_wave", "fisheye_grey_serial", "fisheye_grey_addpoints")


def packaged_from_tracks(tr):
    """the feature map the nodelet builds from the tracker's state (estimator_nodelet.cpp:336-363): track_cnt > 1, ascending id, 7 doubles"""
    ids, cnt, cur, un, vel = tr
    k = np.flatnonzero(cnt > 1)
    k = k[np.argsort(ids[k], kind="stable")]
    obs = np.zeros((len(k), 7))
    obs[:, 0:2] = un[k]; obs[:, 2] = 1.0; obs[:, 3:5] = cur[k]; obs[:, 5:7] = vel[k]
    return ids[k].astype(np.int32), obs


def run_oracle(case, fast_cap=None):
    """The case through the oracle's process_tracker (Pipeline::track) with relative_R = I.  The nodelet drops the very first image it sees
    (estimator_nodelet.cpp:234-240) and vio_track carries no nodelet gating, so frame 0 is shown twice here.  One record per frame:
    tracks (ids, track_cnt, cur, un, vel), trace (None on a SKIP frame: readImage does not run), packaged = (ids, obs) as the nodelet would
    queue it (empty unless PUBLISH), track_out = what Pipeline::track returned (empty on the first two PUBLISH frames: init_pub, init_feature)"""
    o = vio_ct.OraclePipeline(case.cfg)
    o.set_fisheye_mask(case.fisheye)
    o.set_fast_cap(case.fast_cap if fast_cap is None else fast_cap)
    o.track(case.frames[0], case.stamps[0] - DT, PUBLISH, np.eye(3))
    recs = []
    for g, t, m in zip(case.frames, case.stamps, case.modes):
        out = o.track(g, t, m, np.eye(3))
        tr = tuple(a.copy() for a in o.tracks())
        pk = packaged_from_tracks(tr) if m == PUBLISH else (np.zeros(0, np.int32), np.zeros((0, 7)))
        recs.append(dict(tracks=tr, trace=o.tracker_trace() if m != SKIP else None, packaged=pk, track_out=out, mode=m))
    return recs


_cache = {}


def oracle_run(name, P):
    """(case, records), computed once per process and shared by the tests; treat as read-only"""
    if name not in _cache:
        c = build(name, P)
        _cache[name] = (c, run_oracle(c))
    return _cache[name]
