"""Pins the inputs of tests/test_gpu_frontend_edges.py with the oracle alone, so that the GPU comparisons cannot pass vacuously: the
walk-out pairs really make LK travel further than its cached region, the binary pair really tracks, the noise ROI really overflows the
FAST capacity, the near-flat images really fall on both sides of the eigenvalue threshold -- and the pyramid depth follows
cv::buildOpticalFlowPyramid (oracle/frontend.cpp lk_effective_level).  Every bound is a property the input is built to have, with the
figure of the oracle on an x86-64 CPU beside it."""
import numpy as np
import pytest

import frontend_cases as fc
import vio_ct


def _lk(orc, g0, g1, max_level, prev, init=None):
    H, W = g0.shape
    nxt = np.ascontiguousarray(prev if init is None else init, np.float32).copy()
    st = np.zeros(len(prev), np.uint8)
    orc.ovio_lk(g0.ctypes.data, g1.ctypes.data, W, H, max_level, len(prev), prev.ctypes.data, nxt.ctypes.data, st.ctypes.data, 1)
    return nxt, st


def _tracked(nxt, st, prev, shift):
    return int(((st > 0) & (np.abs(nxt - prev - np.float32(shift)).max(1) < 0.5)).sum())


@pytest.mark.parametrize("size", [(333, 241), (322, 246)])
def test_walk_out_pair_travels_beyond_the_cached_region(orc, size):
    """max_level 0, initial flow = previous points, true shift (7, -6): at least half of the 96 grid points must converge on the shift,
    i.e. end more than LK_MARGIN = 5 px from where they started (74 and 76 here)"""
    W, H = size
    g0, g1 = fc.texture_pair(W, H, 7, -6)
    prev = fc.grid_points(W, H)
    nxt, st = _lk(orc, g0, g1, 0, prev)
    good = (st > 0) & (np.abs(nxt - prev - np.float32([7, -6])).max(1) < 0.5)
    assert good.sum() >= 48, int(good.sum())
    assert (np.abs(nxt[good] - prev[good]).max(1) > 5.0).all()


def test_deep_pyramid_follows_a_large_shift(orc):
    """the same texture shifted by (19, 13) at max_level 3: most points follow it (88 of 96 here)"""
    W, H = 333, 241
    g0, g1 = fc.texture_pair(W, H, 19, 13)
    prev = fc.grid_points(W, H)
    nxt, st = _lk(orc, g0, g1, 3, prev)
    assert _tracked(nxt, st, prev, (19, 13)) >= 48


@pytest.mark.parametrize("size", [(333, 241), (644, 484)])
def test_binary_pair_tracks(orc, size):
    """0 / 255 blocks shifted by (-2, 1), max_level 1: at least 90 of 96 within 0.5 px (96 here), on an image whose Scharr sums reach 4080"""
    W, H = size
    g0, g1 = fc.binary_pair(W, H)
    prev = fc.grid_points(W, H)
    nxt, st = _lk(orc, g0, g1, 1, prev)
    assert _tracked(nxt, st, prev, fc.BINARY_SHIFT) >= 90
    I = g0.astype(np.int32)
    ix = 3 * (I[:-2, 2:] - I[:-2, :-2]) + 10 * (I[1:-1, 2:] - I[1:-1, :-2]) + 3 * (I[2:, 2:] - I[2:, :-2])
    assert np.abs(ix).max() == 4080


@pytest.mark.parametrize("W", [333, 336])
def test_noise_roi_overflows_the_fast_capacity(orc, W):
    """113 x 99 ROIs of the noise image hold more than VIO_FAST_CAP = 1024 corners (1067 / 1052 and 1068 / 1046 here)"""
    H = 241
    g = fc.noise(W, H)
    out = np.zeros((4096, 3), np.float32)
    for roi in fc.fast_overflow_rois(W, H):
        assert orc.ovio_fast_roi(g.ctypes.data, W, H, *roi, 4096, out.ctypes.data) > 1024, roi
    f = fc.flat(W, H)
    assert orc.ovio_fast_roi(f.ctypes.data, W, H, 0, 0, W, H, 4096, out.ctypes.data) == 0


def test_near_flat_images_fall_on_both_sides_of_the_eigenvalue_threshold(orc):
    """constant image and 1 / 8 ramp: every point rejected; the ramp whose right half has steps of two grey levels: both statuses"""
    W, H = 333, 241
    prev = fc.lk_points(W, H)
    for img in (fc.flat(W, H), fc.ramp(W, H)):
        assert _lk(orc, img, img, 1, prev)[1].sum() == 0
    img = fc.ramp(W, H, split=True)
    st = _lk(orc, img, img, 1, prev)[1]
    assert 20 <= st[:96].sum() <= 76, int(st[:96].sum())


SMALL = [((64, 64), 1), ((101, 67), 1), ((160, 120), 2)]


@pytest.mark.parametrize("size,eff", SMALL)
def test_small_images_use_the_effective_pyramid_depth(orc, size, eff):
    """max_level 3 on an image whose deeper levels would be 21 px or less is the call with the effective level, bit for bit"""
    W, H = size
    assert fc.effective_level(W, H, 3) == eff
    g0, g1 = fc.texture_pair(W, H, 3, -2)
    prev = fc.lk_points(W, H)
    a, sa = _lk(orc, g0, g1, 3, prev)
    b, sb = _lk(orc, g0, g1, eff, prev)
    assert np.array_equal(sa, sb) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert _tracked(a[:96], sa[:96], prev[:96], (3, -2)) >= 48
    if eff > 1:   # and the effective level is really used: one level fewer gives another answer
        c, sc = _lk(orc, g0, g1, eff - 1, prev)
        assert not np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_smallest_legal_coarsest_level(orc):
    """176 x 176: level 3 is 22 x 22, the smallest level LK may use; all four levels are used (max_level 2 gives another answer)"""
    W = H = 176
    assert fc.level_sizes(W, H)[3] == (22, 22) and fc.effective_level(W, H, 3) == 3
    g0, g1 = fc.texture_pair(W, H, 3, -2)
    prev = fc.coarse_border_points(W, H)
    a, sa = _lk(orc, g0, g1, 3, prev)
    c, sc = _lk(orc, g0, g1, 2, prev)
    assert sa.sum() >= len(prev) // 4
    assert not np.array_equal(a.view(np.uint32), c.view(np.uint32))


# (width, height, max_level) -> effective level, worked out by hand from level = (n + 1) / 2 per step and "every level >= 22 px":
# 41, 42 -> 21 (no level 1); 43, 44 -> 22; 45 -> 23;  168 -> 84, 42, 21;  169 -> 85, 43, 22;  175, 176 -> 88, 44, 22;  177 -> 89, 45, 23
LEVEL_TABLE = [
    ((41, 41, 3), 0), ((42, 42, 3), 0), ((43, 43, 3), 1), ((44, 44, 1), 1), ((45, 45, 3), 1), ((640, 42, 3), 0), ((42, 640, 3), 0),
    ((640, 43, 3), 1), ((83, 640, 3), 1), ((84, 640, 3), 1), ((85, 640, 3), 2), ((168, 168, 3), 2), ((169, 169, 3), 3), ((168, 169, 3), 2), ((169, 168, 3), 2),
    ((175, 175, 3), 3), ((176, 176, 3), 3), ((177, 177, 3), 3), ((176, 176, 2), 2), ((176, 176, 0), 0), ((64, 64, 3), 1), ((101, 67, 3), 1),
    ((160, 120, 3), 2), ((640, 480, 3), 3), ((640, 480, 1), 1), ((848, 480, 3), 3), ((1280, 720, 3), 3), ((333, 241, 3), 3),
]


def test_effective_level_table(P, orc):
    for (W, H, m), want in LEVEL_TABLE:
        assert fc.effective_level(W, H, m) == want, (W, H, m)
        assert orc.ovio_lk_effective_level(W, H, m) == want, (W, H, m)
        assert P.lib().vio_lk_effective_level(W, H, m) == want, (W, H, m)


def test_oracle_tracker_at_160x120_ignores_the_illegal_level(P):
    """the input of the production-kernel GPU test: FeatureTracker::readImage over 12 frames of two sequences at 160 x 120 with
    lk_max_level 3 equals the run with lk_max_level 2, and keeps at least 30 features tracked throughout (74 and more here)"""
    runs = []
    for lvl in (3, 2):
        cfg = fc.small_tracker_config(P, lvl)
        assert cfg.lk_max_level == lvl
        runs.append([fc.run_oracle_tracker(P, cfg, seq) for seq in fc.SMALL_TRACKER_SEQS])
    for a, b in zip(*runs):
        for fa, fb in zip(a, b):
            assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
        assert len(a[-1][0]) >= 30 and int((a[-1][1] >= 8).sum()) >= 30
