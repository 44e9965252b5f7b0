"""The front-end kernels (csrc/fe_kernels.hip) at the sizes, positions and values where their hand-written staging code changes path,
against the CPU oracle on identical inputs (tests/frontend_cases.py; tests/test_frontend_edges_cpu.py pins what those inputs provoke).
Every stage here is integer / fixed-point arithmetic followed by the oracle's float operations one by one: all comparisons are bit-exact."""
import ctypes as C

import numpy as np
import pytest

import frontend_cases as fc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ LK
def _lk_oracle(orc, g0, g1, max_level, prev, init):
    H, W = g0.shape
    a, sa = init.copy(), np.zeros(len(prev), np.uint8)
    orc.ovio_lk(g0.ctypes.data, g1.ctypes.data, W, H, max_level, len(prev), prev.ctypes.data, a.ctypes.data, sa.ctypes.data, 1)
    return a, sa


def _lk_device(P, g0, g1, max_level, prev, init):
    H, W = g0.shape
    b, sb = init.copy(), np.zeros(len(prev), np.uint8)
    assert P.lib().vio_stage_lk(g0.ctypes.data, g1.ctypes.data, W, H, max_level, len(prev), prev.ctypes.data, b.ctypes.data, sb.ctypes.data) == 0
    return b, sb


def _lk_same(P, orc, what, g0, g1, max_level, prev, init=None):
    """vio_stage_lk against ovio_lk: status equal point for point, positions the same floats; returns the oracle's (positions, status)"""
    prev = np.ascontiguousarray(prev, np.float32)
    init = prev.copy() if init is None else np.ascontiguousarray(init, np.float32)
    a, sa = _lk_oracle(orc, g0, g1, max_level, prev, init)
    b, sb = _lk_device(P, g0, g1, max_level, prev, init)
    H, W = g0.shape
    bad = np.flatnonzero((sa != sb) | (a.view(np.uint32) != b.view(np.uint32)).any(1))
    assert len(bad) == 0, "%s %dx%d max_level %d: %d of %d points differ, first %d: prev %s init %s oracle %s status %d device %s status %d" % (
        what, W, H, max_level, len(bad), len(prev), bad[0], prev[bad[0]], init[bad[0]], a[bad[0]], sa[bad[0]], b[bad[0]], sb[bad[0]])
    return a, sa


def _outside_guesses(prev, W, H, d):
    """initial guesses d px beyond the left / right / top / bottom border, a quarter of the points each"""
    init = prev.copy()
    k = np.arange(len(prev)) % 4
    init[k == 0, 0] = -d
    init[k == 1, 0] = W - 1 + d
    init[k == 2, 1] = -d
    init[k == 3, 1] = H - 1 + d
    return init


LK_SIZES = [(333, 241),   # odd at every level
            (322, 246),   # even, never a multiple of 4: the byte path everywhere
            (424, 240),   # a multiple of 4 at level 0 only (212, 106, 53 follow)
            (644, 484)]   # aligned at levels 0 and 1, 161 at level 2


@pytest.mark.parametrize("size", LK_SIZES)
def test_lk_staging_paths(P, orc, size):
    """max_level 0..3 on each size, 96 grid points plus the explicit border points (fc.border_points: ipx on both sides of -WIN and w,
    template blocks across the last aligned column).  Initial flow = previous points on a pair shifted by (7, -6): at max_level 0 the
    iteration leaves the 32 x 32 cached region and re-centres it; (19, 13) at max_level 3; guesses 40 and 500 px outside the image
    (reg_ok false when the level starts)."""
    W, H = size
    prev = fc.lk_points(W, H)
    g0, g1 = fc.texture_pair(W, H, 7, -6)
    for ml in range(4):
        a, sa = _lk_same(P, orc, "walk-out", g0, g1, ml, prev)
        good = (sa[:96] > 0) & (np.abs(a[:96] - prev[:96] - np.float32([7, -6])).max(1) < 0.5)
        assert good.sum() >= 48, (ml, int(good.sum()))
        for d in (40, 500):
            _, so = _lk_same(P, orc, "guess %d px outside" % d, g0, g1, ml, prev, _outside_guesses(prev, W, H, d))
            if d == 500:
                assert so.sum() == 0
    h0, h1 = fc.texture_pair(W, H, 19, 13)
    a, sa = _lk_same(P, orc, "shift (19, 13)", h0, h1, 3, prev)
    assert ((sa[:96] > 0) & (np.abs(a[:96] - prev[:96] - np.float32([19, 13])).max(1) < 0.5)).sum() >= 48


@pytest.mark.parametrize("size", LK_SIZES)
def test_lk_integer_extremes_and_flat_patches(P, orc, size):
    """0 / 255 blocks: Scharr sums of 4080 and patch differences of 8160, the bounds the 24-bit multiplies and the 32-bit wave sums are
    argued from.  Constant image and shallow ramps: the minEig / D rejection, equal point for point, with both outcomes present."""
    W, H = size
    prev = fc.lk_points(W, H)
    g0, g1 = fc.binary_pair(W, H)
    for ml in (1, 3):
        a, sa = _lk_same(P, orc, "binary", g0, g1, ml, prev)
        assert ((sa[:96] > 0) & (np.abs(a[:96] - prev[:96] - np.float32(fc.BINARY_SHIFT)).max(1) < 0.5)).sum() >= 90
    _lk_same(P, orc, "binary, far guesses", g0, g1, 0, prev, prev + np.float32([6, 5]))
    seen = set()
    for name, img in (("flat", fc.flat(W, H)), ("ramp", fc.ramp(W, H)), ("split ramp", fc.ramp(W, H, split=True))):
        for ml in (0, 1):
            _, st = _lk_same(P, orc, name, img, img, ml, prev)
            seen |= set(st.tolist())
        if name != "split ramp":
            assert st.sum() == 0
    assert seen == {0, 1}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_lk_point_counts(P, orc, n):
    W, H = 333, 241
    g0, g1 = fc.texture_pair(W, H, 3, -2)
    prev = fc.lk_points(W, H)[:n]
    a, sa = _lk_same(P, orc, "n = %d" % n, g0, g1, 1, prev)
    assert len(a) == n and (n == 0 or sa.sum() > 0)


@pytest.mark.parametrize("size,eff", [((64, 64), 1), ((101, 67), 1), ((160, 120), 2)])
def test_lk_small_images_use_the_effective_depth(P, orc, size, eff):
    """cv::buildOpticalFlowPyramid stops before the first level of 21 px or less: max_level 3 is the call with the effective level, bit
    for bit, on the device and in the oracle, and the two agree"""
    W, H = size
    assert P.lib().vio_lk_effective_level(W, H, 3) == eff == fc.effective_level(W, H, 3)
    g0, g1 = fc.texture_pair(W, H, 3, -2)
    prev = fc.lk_points(W, H)
    a3, s3 = _lk_same(P, orc, "small, max_level 3", g0, g1, 3, prev)
    ae, se = _lk_same(P, orc, "small, effective level", g0, g1, eff, prev)
    assert np.array_equal(s3, se) and np.array_equal(a3.view(np.uint32), ae.view(np.uint32))
    b3, t3 = _lk_device(P, g0, g1, 3, prev, prev.copy())
    be, te = _lk_device(P, g0, g1, eff, prev, prev.copy())
    assert np.array_equal(t3, te) and np.array_equal(b3.view(np.uint32), be.view(np.uint32))
    assert ((s3[:96] > 0) & (np.abs(a3[:96] - prev[:96] - np.float32([3, -2])).max(1) < 0.5)).sum() >= 48


def test_lk_smallest_legal_coarsest_level(P, orc):
    """176 x 176: level 3 is 22 x 22, where -21 reflects to 21 and w + 20 to w - 22, the last pixels one reflection reaches.  All four
    levels are used (max_level 2 gives other positions), with points on the first / last pixel of the coarsest level at all four borders."""
    W = H = 176
    assert P.lib().vio_lk_effective_level(W, H, 3) == 3
    g0, g1 = fc.texture_pair(W, H, 3, -2)
    prev = np.ascontiguousarray(np.vstack([fc.coarse_border_points(W, H), fc.border_points(W, H)]), np.float32)
    a3, s3 = _lk_same(P, orc, "176", g0, g1, 3, prev)
    a2, s2 = _lk_same(P, orc, "176", g0, g1, 2, prev)
    assert not np.array_equal(a3.view(np.uint32), a2.view(np.uint32))
    assert s3.sum() >= 9


# ------------------------------------------------------------------------------------------------ pyrDown
# an aligned interior tile of pyrdown_tile needs sw >= 260 (tile column 1 stages source columns 124 .. 259), sh >= 65 (tile row 1 stages
# rows 30 .. 64) and sw % 4 == 0
PYR_SIZES = [(256, 67), (260, 64),            # no aligned tile: too narrow / too low by one step
             (260, 65),                       # exactly one, flush with the right and the bottom edge
             (264, 68), (388, 97),            # one and a partial / several
             (261, 65),                       # the same extent on the byte path
             (132, 36), (136, 35),
             (23, 22), (8, 8), (3, 3), (64, 3), (3, 64)]   # the smallest sizes a single reflection serves


@pytest.mark.parametrize("kind", ["noise", "binary", "texture"])
def test_pyr_down_tile_paths(P, orc, kind):
    """vio_stage_pyr_down against ovio_pyr_down.  Not covered, and not coverable through this entry: a source pointer that is not 4-byte
    aligned (the stage entry copies the image into a hipMalloc allocation, which is aligned; the pipeline's own buffers are too)."""
    make = {"noise": fc.noise, "binary": fc.binary, "texture": fc.texture}[kind]
    for (W, H) in PYR_SIZES:
        img = make(W, H)
        ref = np.zeros(((H + 1) // 2, (W + 1) // 2), np.uint8)
        out = np.full_like(ref, 0xA5)
        orc.ovio_pyr_down(img.ctypes.data, W, H, ref.ctypes.data)
        assert P.lib().vio_stage_pyr_down(img.ctypes.data, W, H, out.ctypes.data) == 0
        bad = np.argwhere(ref != out)
        assert len(bad) == 0, "%s %dx%d: %d pixels differ, first (x, y) = (%d, %d): oracle %d device %d" % (
            kind, W, H, len(bad), bad[0][1], bad[0][0], ref[tuple(bad[0])], out[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ FAST
def _fast_rois(W, H):
    r = [(0, 0, 40, 30), (1, 2, 41, 31), (2, 1, 42, 30), (3, 3, 43, 33)]           # lead-in xo = 0 .. 3, rw % 4 = 0 .. 3
    r += [(W - 45, H - 33, 45, 33), (W - 40, 5, 40, 30), (6, H - 30, 42, 30)]       # flush with the right / bottom edges
    r += [(10, 20, 7, 7), (W - 7, H - 7, 7, 7)]                                     # one interior pixel
    r += [(5, 9, 110, 8), (9, 5, 8, 110)]
    r += [(17, 11, 14, 14), (18, 12, 11, 19), (19, 13, 22, 10)]                     # 64, 65 and 64 interior pixels: the ballot-word boundary
    r += [(0, 0, 113, 99)]
    return r


@pytest.mark.parametrize("kind", ["noise", "binary", "texture"])
@pytest.mark.parametrize("W", [333, 336])
def test_fast_roi_edges(P, orc, W, kind):
    """vio_stage_fast_roi against ovio_fast_roi: W = 333 stages the ROI byte by byte, W = 336 with aligned 4-byte loads from the
    column r.x & ~3"""
    H = 241
    img = {"noise": fc.noise, "binary": fc.binary, "texture": lambda w, h: fc.texture(w, h, sigma=1.0)}[kind](W, H)
    cap, total = 4096, 0
    for roi in _fast_rois(W, H):
        a, b = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
        na = orc.ovio_fast_roi(img.ctypes.data, W, H, *roi, cap, a.ctypes.data)
        nb = P.lib().vio_stage_fast_roi(img.ctypes.data, W, H, *roi, cap, b.ctypes.data)
        assert na == nb, (roi, na, nb)
        assert np.array_equal(a[:na], b[:nb]), (roi, int(np.flatnonzero((a[:na] != b[:na]).any(1))[0]))
        total += na
    assert total > 100
    flat = fc.flat(W, H)
    assert P.lib().vio_stage_fast_roi(flat.ctypes.data, W, H, 0, 0, 113, 99, cap, b.ctypes.data) == 0


@pytest.mark.parametrize("W", [333, 336])
def test_fast_more_survivors_than_cap(P, orc, W):
    """more corners than the output holds (cap = VIO_FAST_CAP = 1024, and cap = 1): the count is the total, the first cap entries are the
    oracle's first cap in raster order, nothing is written beyond them"""
    H = 241
    img = fc.noise(W, H)
    for roi in fc.fast_overflow_rois(W, H):
        full = np.zeros((4096, 3), np.float32)
        n = orc.ovio_fast_roi(img.ctypes.data, W, H, *roi, 4096, full.ctypes.data)
        assert n > 1024
        order = full[:n, 1] * 4096 + full[:n, 0]
        assert (np.diff(order) > 0).all()
        for cap in (1024, 1):
            out = np.full((cap + 64, 3), -7.0, np.float32)
            assert P.lib().vio_stage_fast_roi(img.ctypes.data, W, H, *roi, cap, out.ctypes.data) == n, (roi, cap)
            assert np.array_equal(out[:cap], full[:cap]), (roi, cap)
            assert (out[cap:] == -7.0).all(), (roi, cap)


# ------------------------------------------------------------------------------------------------ RANSAC
def _ransac_same(P, orc, cfg, p1, p2):
    n = len(p1)
    p1, p2 = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    sa, sb = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
    orc.ovio_ransac(C.byref(cfg), n, p1.ctypes.data, p2.ctypes.data, sa.ctypes.data)
    assert P.lib().vio_stage_ransac(C.byref(cfg), n, p1.ctypes.data, p2.ctypes.data, sb.ctypes.data) == 0
    assert np.array_equal(sa, sb), (n, sa.tolist(), sb.tolist())
    return sa


def test_ransac_small_and_degenerate_sets(P, orc):
    """n around the 8-point minimum and around the wavefront width; collinear and coincident points.  Both sides refuse n < 8
    (rejectWithF, feature_tracker.cpp:443: `if (forw_pts.size() >= 8)`): every status 0."""
    cfg = P.default_config()
    p1, p2, bad = fc.two_view_scene(150)
    for n in (7, 8, 9, 63, 64, 65):
        st = _ransac_same(P, orc, cfg, p1[:n], p2[:n])
        assert set(st.tolist()) <= {0, 1}
        if n == 7:
            assert st.sum() == 0
        if n >= 63:
            assert st.sum() >= n // 2 and st[bad[bad < n]].sum() <= 2
    t = np.linspace(0, 1, 40, dtype=np.float32)[:, None]
    line = np.float32([50, 60]) + t * np.float32([500, 330])
    _ransac_same(P, orc, cfg, line, line + np.float32([3.5, -1.25]))
    _ransac_same(P, orc, cfg, line, line)
    same = np.tile(np.float32([[321.5, 200.25]]), (40, 1))
    _ransac_same(P, orc, cfg, same, same)
    _ransac_same(P, orc, cfg, same, same + np.float32([2, 1]))


# ------------------------------------------------------------------------------------------------ the production kernels
def test_production_kernels_at_160x120_use_the_effective_depth(P):
    """fe_pyrdown / fe_lk / fe_select / fe_fast / fe_add over 12 frames of two sequences at 160 x 120 with lk_max_level 3 (levels 80 x 60,
    40 x 30, 20 x 15: the last one illegal): the tracker state after every frame equals the oracle's bit for bit, and equals the same
    run configured with lk_max_level 2 -- the derived depth in DevCfg, which only the batch kernels read."""
    seqs = fc.SMALL_TRACKER_SEQS
    runs = {}
    for lvl in (3, 2):
        cfg = fc.small_tracker_config(P, lvl)
        frames = [fc.small_tracker_frames(P, cfg, s) for s in seqs]
        b = P.VioBatch(cfg, len(seqs))
        out = [[] for _ in seqs]
        for f, t in enumerate(fc.SMALL_TRACKER_TIMES):
            b.track(np.stack([frames[i][f] for i in range(len(seqs))]), [t] * len(seqs), publish=True)
            for i in range(len(seqs)):
                out[i].append(tuple(x.copy() for x in b.tracks(i)))
        b.close()
        runs[lvl] = out
    cfg = fc.small_tracker_config(P, 3)
    for i, s in enumerate(seqs):
        ref = fc.run_oracle_tracker(P, cfg, s)
        for f in range(len(ref)):
            for k in range(5):
                x, y, z = ref[f][k], runs[3][i][f][k], runs[2][i][f][k]
                assert x.shape == y.shape == z.shape, (s, f, k, x.shape, y.shape, z.shape)
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (s, f, k)
                assert np.array_equal(y.view(np.uint32), z.view(np.uint32)), (s, f, k)
        assert len(ref[-1][0]) >= 30 and int((ref[-1][1] >= 8).sum()) >= 30
