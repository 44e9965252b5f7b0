"""Deterministic input images and point sets for the front-end edge tests (test_frontend_edges_cpu.py pins them with the oracle alone,
test_gpu_frontend_edges.py runs the kernels on them).  Plain numpy, no GPU, fixed seeds."""
import numpy as np

PAD = 32   # a texture canvas is 2 * PAD larger than the image: room for integer shifts of up to PAD px in any direction


def _canvas(W, H, seed, sigma):
    """standard normal noise on (H + 64) x (W + 64), Gaussian low-pass exp(-2 (pi sigma)^2 (fx^2 + fy^2)) in the Fourier domain, unit
    standard deviation, clip(128 + 60 s, 0, 255) as uint8"""
    rng = np.random.default_rng(seed)
    h, w = H + 2 * PAD, W + 2 * PAD
    z = rng.standard_normal((h, w))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    s = np.real(np.fft.ifft2(np.fft.fft2(z) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))))
    s /= s.std()
    return np.clip(128.0 + 60.0 * s, 0, 255).astype(np.uint8)


def _crop(c, W, H, dx=0, dy=0):
    """the W x H crop in which the canvas content sits (dx, dy) px further right / down than in the centred crop"""
    assert abs(dx) <= PAD and abs(dy) <= PAD
    return np.ascontiguousarray(c[PAD - dy:PAD - dy + H, PAD - dx:PAD - dx + W])


def texture(W, H, seed=1, sigma=3.0):
    return _crop(_canvas(W, H, seed, sigma), W, H)


def texture_pair(W, H, dx, dy, seed=1, sigma=3.0):
    """(prev, next) with next(x + dx, y + dy) == prev(x, y) wherever both crops see the canvas: the true flow is exactly (dx, dy)"""
    c = _canvas(W, H, seed, sigma)
    return _crop(c, W, H), _crop(c, W, H, dx, dy)


def _binary_canvas(W, H, seed):
    rng = np.random.default_rng(seed)
    h, w = H + 2 * PAD, W + 2 * PAD
    b = rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3), dtype=np.uint8) * np.uint8(255)
    return np.kron(b, np.ones((3, 3), np.uint8))[:h, :w]


def binary(W, H, seed=2):
    """random 0 / 255 blocks of 3 x 3 px: the largest Scharr sums (|Ix| = 4080) and patch differences a uint8 image can give"""
    return _crop(_binary_canvas(W, H, seed), W, H)


BINARY_SHIFT = (-2, 1)


def binary_pair(W, H, seed=2):
    c = _binary_canvas(W, H, seed)
    return _crop(c, W, H), _crop(c, W, H, *BINARY_SHIFT)


def noise(W, H, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def flat(W, H, value=77):
    return np.full((H, W), value, np.uint8)


def ramp(W, H, split=False):
    """steps of one grey level every 8 px in x and in y (slope 1 / 8 per px each way).  Scharr sums are 0 except +-16 beside a step, and a
    21 x 21 window holds so few steps that its smallest eigenvalue is about half of calcOpticalFlowPyrLK's 1e-4 threshold: every point is
    rejected.  split: right of the middle column the steps are two grey levels high (four times the eigenvalue, about twice the
    threshold), so windows left of, across and right of the seam fall on both sides of the threshold in one image."""
    yy, xx = np.mgrid[0:H, 0:W]
    r = xx // 8 + yy // 8
    if split:
        r = np.where(xx >= W // 2, 2 * r, r)
    return (r % 256).astype(np.uint8)


def grid_points(W, H, n=96, margin=30, seed=11):
    """n points on a 12-column grid `margin` px inside the image, at random sub-pixel offsets"""
    cols = 12
    rows = (n + cols - 1) // cols
    xs = np.linspace(margin, W - 1 - margin, cols)
    ys = np.linspace(margin, H - 1 - margin, rows)
    p = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)[:n]
    p = np.floor(p) + np.random.default_rng(seed).uniform(0, 1, p.shape)
    return np.ascontiguousarray(p, np.float32)


def border_points(W, H):
    """previous points on both sides of every bounds test of the LK window (ipx = floor(x - 10) against -21 and w, likewise in y), and
    points whose 24-wide template block (columns floor(x) - 11 .. floor(x) + 12) straddles the last 4-byte aligned column of the image"""
    ex = [-11.5, -10.5, 0.0, 0.5, W - 1.0, W + 9.5, W + 10.5]
    ey = [-11.5, -10.5, 0.0, 0.5, H - 1.0, H + 9.5, H + 10.5]
    p = [(x, H * 0.5 + 0.25) for x in ex] + [(W * 0.5 + 0.25, y) for y in ey] + list(zip(ex, ey)) + list(zip(ex, ey[::-1]))
    p += [(W - 12.0 + k + 0.25, H * (0.3 + 0.1 * k)) for k in range(4)]      # x = W - 12 .. W - 9
    p += [(W * (0.3 + 0.1 * k), H - 12.0 + k + 0.75) for k in range(4)]
    return np.ascontiguousarray(np.array(p), np.float32)


def lk_points(W, H):
    """the 96 grid points followed by the explicit border points"""
    return np.ascontiguousarray(np.vstack([grid_points(W, H), border_points(W, H)]), np.float32)


def level_sizes(W, H, levels=3):
    out = [(W, H)]
    for _ in range(levels):
        W, H = (W + 1) // 2, (H + 1) // 2
        out.append((W, H))
    return out


def effective_level(W, H, max_level, win=21):
    """cv::buildOpticalFlowPyramid's stopping rule, restated independently of the code under test: the deepest level l <= max_level such
    that every level 1..l exceeds the window in width and height"""
    lv = 0
    for (w, h) in level_sizes(W, H, max_level)[1:]:
        if w <= win or h <= win:
            break
        lv += 1
    return lv


def coarse_border_points(W, H):
    """6 x 6 points from 1.5 px inside one border to 1.5 px inside the other: at a 22 x 22 coarsest level the outer ones sit on its
    first / last pixel in x, in y and in both, so their windows reflect at all four borders (and both reflect at once in the corners)"""
    xs = np.array([1.5, 0.12 * W, 0.35 * W, 0.65 * W, 0.88 * W, W - 2.5]) + 0.3
    ys = np.array([1.5, 0.12 * H, 0.35 * H, 0.65 * H, 0.88 * H, H - 2.5]) + 0.6
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2), np.float32)


def fast_overflow_rois(W, H):
    """113 x 99 ROIs (the 640 x 480 grid's cell size) at the top-left corner (lead-in 0) and flush with the right and bottom edges"""
    return [(0, 0, 113, 99), (W - 113, H - 99, 113, 99)]


# ---- the production kernels at a size whose level 3 is illegal (160 x 120: 80 x 60, 40 x 30, 20 x 15)
SMALL_TRACKER_SEQS = (5, 6)
SMALL_TRACKER_TIMES = 2.0 + np.arange(12) * 0.1


def small_tracker_config(P, lk_max_level):
    """the default configuration scaled to 160 x 120, with min_dist / max_cnt reduced so that the small image still carries 70+ tracks"""
    d = P.default_config()
    return P.default_config(width=160, height=120, fx=d.fx / 4, fy=d.fy / 4, cx=d.cx / 4, cy=d.cy / 4, lk_max_level=lk_max_level,
                            min_dist=6, max_cnt=100)


def small_tracker_frames(P, cfg, seq):
    import vio_ct
    syn = P.Synth(vio_ct.synth_like(cfg))
    return [syn.render_host(seq, t)[0] for t in SMALL_TRACKER_TIMES]


def run_oracle_tracker(P, cfg, seq):
    """FeatureTracker::readImage (relative_R = I, publishing) over the frames of `seq`: the tracker's (ids, track_cnt, cur, un, velocity) after every frame"""
    import vio_ct
    ot = vio_ct.OracleTracker(cfg)
    out = []
    for g, t in zip(small_tracker_frames(P, cfg, seq), SMALL_TRACKER_TIMES):
        ot.read(g, t, None, True)
        out.append(tuple(x.copy() for x in ot.tracks()))
    return out


def two_view_scene(n=150, seed=1):
    """the two-view scene of tests/test_gpu_stages.py::test_ransac_same_inliers: n points 2 .. 6 m in front of a camera (f = 460,
    c = (320, 240)) that turns by 0.05 rad and moves by (0.15, 0.02, 0.05) m, 0.2 px noise, every sixth correspondence an outlier of
    8 .. 30 px.  Returns (p1, p2, outlier indices)."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 6, n)]
    th = 0.05
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    X2 = (R @ X.T).T + np.array([0.15, 0.02, 0.05])
    p1 = np.ascontiguousarray((460 * X[:, :2] / X[:, 2:3] + [320, 240]).astype(np.float32))
    p2 = np.ascontiguousarray((460 * X2[:, :2] / X2[:, 2:3] + [320, 240]).astype(np.float32))
    p2 += rng.normal(0, 0.2, p2.shape).astype(np.float32)
    bad = np.sort(rng.choice(n, n // 6, replace=False))
    p2[bad] += rng.uniform(8, 30, (len(bad), 2)).astype(np.float32)
    return p1, p2, bad
