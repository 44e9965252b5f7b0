"""The pose-graph kernels (csrc/pg_kernels.hip, csrc/pg_bow.hip) at the sizes, positions and values where their hand-written tiles, halos,
ballots and wave-wide arg-min reductions change path, against the CPU oracle on identical inputs and -- where the image is small enough
for numpy -- against the plain definitions of tests/posegraph_cases.py (tests/test_posegraph_edges_cpu.py pins what those inputs
provoke).  Every operation is integer arithmetic, or IEEE double arithmetic rounded once to float: all comparisons are bit-exact."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import bow_util
import posegraph_cases as pc
import test_oracle_posegraph_cpu as O
import vio_ct

pytestmark = pytest.mark.gpu

NONE = np.zeros((0, 2), np.float32)


@pytest.fixture(scope="module")
def PG(P):
    return importlib.import_module("vins-rgbd-fast_amd.posegraph")


@pytest.fixture(scope="module")
def L(PG):
    return PG._lib()[1]   # the C ABI with the vio_pg_* argument types bound


@functools.lru_cache(maxsize=None)
def _oracle_blur(kind, W, H):
    img = pc.image(kind, W, H)
    out = np.zeros_like(img)
    O.olib().ovio_pg_blur(img.ctypes.data, W, H, out.ctypes.data)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_describe(kind, W, H, thr):
    """(window descriptors, keypoints, their descriptors, their normalised coordinates) of the oracle, computed once and shared"""
    cfg = vio_ct.pkg().canonical_config(width=W, height=H)
    return O.o_describe(cfg, pc.image(kind, W, H), pc.all_window_points(W, H), pc.pattern(), thr, cap=100000)


def _first_diff(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return None if len(bad) == 0 else tuple(int(v) for v in bad[0])


# ------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_blur_partial_tiles_and_halos(P, L, size):
    """vio_pg_stage_blur against ovio_pg_blur and blur_def: tiles cut by the right and the bottom edge, and tiles whose halo reflects
    at both sides at once (W = 16, 17: columns -4 and W + 3 of one tile).  A constant image stays constant."""
    W, H = size
    for kind in pc.KINDS + ("flat",):
        img = pc.image(kind, W, H)
        out = np.full_like(img, 0xA5)
        assert L.vio_pg_stage_blur(img.ctypes.data, W, H, out.ctypes.data) == 0
        for name, ref in (("oracle", _oracle_blur(kind, W, H)), ("definition", pc.blur_def(img))):
            bad = _first_diff(out, ref)
            assert bad is None, "%s %dx%d against the %s: %d pixels differ, first (x, y) = (%d, %d): expected %d, device %d" % (
                kind, W, H, name, int((out != ref).sum()), bad[1], bad[0], ref[bad], out[bad])
        if kind == "flat":
            assert (out == 77).all()


# ------------------------------------------------------------------------------------------------ keypoints and descriptors
@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_keypoints_and_descriptors(P, PG, size, kind):
    """posegraph.describe at FAST thresholds 1, 20 and 254 with window points inside, near, on and beyond every border: the keypoint
    list (count, order), the window and keypoint descriptors and the normalised keypoints equal the oracle's; on the sizes up to
    200 x 50 they equal the numpy definitions as well.  Threshold 254 on noise / texture is the empty list; 848 x 480 and 1280 x 720
    noise have more keypoints than describe makes room for at first (it must come back with all of them)."""
    W, H = size
    cfg = P.canonical_config(width=W, height=H)
    img, uv, pat = pc.image(kind, W, H), pc.all_window_points(W, H), pc.pattern()
    for thr in pc.THRESHOLDS:
        what = "%s %dx%d threshold %d" % (kind, W, H, thr)
        wd, kxy, kd, kn = PG.describe(cfg, img, uv, pat, fast_threshold=thr)
        wd_o, kxy_o, kd_o, kn_o = _oracle_describe(kind, W, H, thr)
        assert len(kxy) == len(kxy_o), "%s: %d keypoints, the oracle has %d" % (what, len(kxy), len(kxy_o))
        assert np.array_equal(kxy, kxy_o), "%s: keypoint %s differs" % (what, _first_diff(kxy, kxy_o))
        assert wd.dtype == kd.dtype == np.uint64
        assert np.array_equal(wd, wd_o), "%s: window descriptor of point %s differs" % (what, uv[_first_diff(wd, wd_o)[0]])
        assert np.array_equal(kd, kd_o), "%s: descriptor of keypoint %s differs" % (what, kxy[_first_diff(kd, kd_o)[0]])
        assert pc.same_floats(kn, kn_o), what
        if size in pc.SMALL:
            blur = pc.blur_def(img)
            assert np.array_equal(kxy, pc.fast_keypoints_def(img, thr)), what
            assert np.array_equal(wd, pc.brief_def(blur, uv, pat)) and np.array_equal(kd, pc.brief_def(blur, kxy, pat)), what
            assert pc.same_floats(kn, pc.lift_def(cfg, kxy)), what
        if thr == 254 and kind != "binary":
            assert len(kxy) == 0 and kd.shape == (0, 4) and kn.shape == (0, 2)
        else:
            assert len(kxy) > 0


def _describe_raw(L, cfg, img, uv, thr, cap, room, sentinel=True):
    """vio_pg_describe itself (the wrapper retries with a larger cap): outputs with `room` entries, pre-filled with a sentinel"""
    n = len(uv)
    wd = np.full((max(n, 1), 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    kxy, kd, kn = np.full((room, 2), -7.0, np.float32), np.full((room, 4), 0xA5A5A5A5A5A5A5A5, np.uint64), np.full((room, 2), -7.0, np.float32)
    rc = L.vio_pg_describe(C.byref(cfg), img.ctypes.data, n, uv.ctypes.data if n else None, pc.pattern().ctypes.data, thr, wd.ctypes.data if n else None,
                           cap, kxy.ctypes.data, kd.ctypes.data, kn.ctypes.data)
    return rc, wd[:n], kxy, kd, kn


def test_more_keypoints_than_cap(P, L):
    """200 x 50 noise at threshold 20 has 842 keypoints.  With cap = 0, 1, 64, 841, 842, 843 the return value is 842 every time, the first
    min(cap, 842) keypoints, descriptors and normalised points are the full list's prefix, and nothing is written beyond them."""
    W, H = pc.TRUNCATION_SIZE
    thr, total = pc.TRUNCATION_THRESHOLD, pc.TRUNCATION_TOTAL
    cfg = P.canonical_config(width=W, height=H)
    img, uv = pc.image("noise", W, H), pc.all_window_points(W, H)
    wd_o, kxy_o, kd_o, kn_o = _oracle_describe("noise", W, H, thr)
    assert len(kxy_o) == total
    for cap in (0, 1, 64, 841, 842, 843):
        for pts in (uv, NONE):
            rc, wd, kxy, kd, kn = _describe_raw(L, cfg, img, pts, thr, cap, total + 64)
            assert rc == total, (cap, len(pts), rc)
            m = min(cap, total)
            assert np.array_equal(kxy[:m], kxy_o[:m]) and np.array_equal(kd[:m], kd_o[:m]) and pc.same_floats(kn[:m], kn_o[:m]), (cap, len(pts))
            assert (kxy[m:] == -7.0).all() and (kd[m:] == 0xA5A5A5A5A5A5A5A5).all() and (kn[m:] == -7.0).all(), (cap, len(pts))
            if len(pts):
                assert np.array_equal(wd, wd_o), cap
    # the empty list with room for it, and with none
    for cap in (0, 5):
        rc, _, kxy, kd, kn = _describe_raw(L, cfg, img, NONE, 254, cap, 8)
        assert rc == 0 and (kxy == -7.0).all() and (kd == 0xA5A5A5A5A5A5A5A5).all() and (kn == -7.0).all()


# ------------------------------------------------------------------------------------------------ camera lift
def _centred(P, cam, W, H):
    """the lens with its principal point moved to the centre of a W x H image"""
    names = P.CAMERA_PARAMS[cam.model]
    c = P.Camera()
    c.model, c.reserved = cam.model, cam.reserved
    for i in range(12):
        c.p[i] = cam.p[i]
    c.p[names.index("u0")], c.p[names.index("v0")] = W / 2.0, H / 2.0
    return c


@pytest.mark.parametrize("size", [(65, 33), (848, 480)], ids=pc.size_id)
def test_keypoints_through_camera_models(P, PG, size):
    """vio_pg_describe_camera with the Kannala-Brandt and MEI lenses: kp_norm is vio_stage_host_camera's lift of the same keypoints
    rounded to float32; keypoints and descriptors do not depend on the lens"""
    from test_gpu_camera_models import _lenses
    W, H = size
    cfg = P.canonical_config(width=W, height=H)
    img, uv, pat = pc.image("noise", W, H), pc.all_window_points(W, H), pc.pattern()
    wd_o, kxy_o, kd_o, kn_o = _oracle_describe("noise", W, H, 20)
    kb, mei, _ = _lenses(P)
    seen = []
    for cam in (_centred(P, kb, W, H), _centred(P, mei, W, H)):
        wd, kxy, kd, kn = PG.describe(cfg, img, uv, pat, camera=cam, cap=40000)
        assert np.array_equal(kxy, kxy_o) and np.array_equal(wd, wd_o) and np.array_equal(kd, kd_o)
        _, un, _ = P.stage_host_camera(cam, kxy.astype(np.float64))
        assert np.isfinite(un).all() and pc.same_floats(kn, un.astype(np.float32)), cam.model
        assert not np.array_equal(kn, kn_o)          # not the configuration's pinhole
        seen.append(kn)
    assert not np.array_equal(seen[0], seen[1])


# ------------------------------------------------------------------------------------------------ Hamming search
def _match_same(PG, a, b, with_def=True):
    """vio_pg_match against ovio_pg_match (and match_def): returns (indices, distances)"""
    bi, bd = PG.match(a, b)
    oi, od = O.o_match(a, b)
    assert np.array_equal(bi, oi) and np.array_equal(bd, od), (len(a), len(b), _first_diff(bi, oi), _first_diff(bd, od))
    if with_def:
        di, dd = pc.match_def(a, b)
        assert np.array_equal(bi, di) and np.array_equal(bd, dd), (len(a), len(b))
    return bi, bd


def test_match_thresholds_and_ties(PG):
    """the all-zero query against one candidate at distance 0, 79, 80, 127, 128, 256: accepted below 80, the distance floored at 128;
    no candidate at all; and the minimum planted in several lanes and several times in one lane: the smallest index wins"""
    q = pc.ZERO.reshape(1, 4)
    for dist, want in pc.SINGLE_CASES:
        bi, bd = _match_same(PG, q, pc.single_candidate(dist))
        assert (int(bi[0]), int(bd[0])) == want, (dist, bi, bd)
    bi, bd = _match_same(PG, q, np.zeros((0, 4), np.uint64))
    assert (int(bi[0]), int(bd[0])) == (-1, 128)
    for b, want in (pc.tie_case_lanes(), pc.tie_case_later_lane()):
        bi, bd = _match_same(PG, q, b)
        assert (int(bi[0]), int(bd[0])) == want
        # the same candidates against 65 queries (the zero query among them at 0 and 64)
        qs = np.array([pc.with_bits(pc.ZERO, k % 64, 130) for k in range(65)], np.uint64)
        bi, bd = _match_same(PG, qs, b)
        assert (int(bi[0]), int(bd[0])) == want == (int(bi[64]), int(bd[64]))


def test_match_counts_around_the_wavefront_width(P, PG):
    """n = 1, 63, 64, 65 queries against m = 0, 1, 63, 64, 65, 127, 128, 129 candidates: keypoint descriptors of two shifted crops of one
    texture, from the device's own describe"""
    W, H = 200, 50
    cfg = P.canonical_config(width=W, height=H)
    g0, g1 = pc.fc.texture_pair(W, H, 2, -1)
    a = PG.describe(cfg, g1, NONE, pc.pattern())[2]
    b = PG.describe(cfg, g0, NONE, pc.pattern())[2]
    assert len(a) >= 65 and len(b) >= 129
    hits = 0
    for n in (1, 63, 64, 65):
        for m in (0, 1, 63, 64, 65, 127, 128, 129):
            bi, bd = _match_same(PG, a[:n], b[:m])
            assert len(bi) == n and (m > 0 or ((bi == -1).all() and (bd == 128).all()))
            hits += int((bi >= 0).sum())
    assert hits > 500
    bi, _ = PG.match(a[:0], b)
    assert len(bi) == 0


def test_match_candidate_count_limit(P, L):
    """the index has 20 bits with 0xFFFFF as the `none` sentinel: m = 0xFFFFE candidates are accepted -- all zero: the first one wins;
    only the last one below 128: its index 0xFFFFD comes back -- and m = 0xFFFFF is VIO_EINVAL"""
    big = np.zeros((0xFFFFF, 4), np.uint64)
    m = 0xFFFFE
    bi, bd = np.full(1, -9, np.int32), np.full(1, -9, np.int32)
    q = pc.ZERO.reshape(1, 4).copy()
    assert L.vio_pg_match(q.ctypes.data, 1, big.ctypes.data, m, bi.ctypes.data, bd.ctypes.data) == 0
    assert (int(bi[0]), int(bd[0])) == (0, 0)
    q = pc.with_bits(pc.ZERO, 200, 11).reshape(1, 4)
    assert L.vio_pg_match(q.ctypes.data, 1, big.ctypes.data, m, bi.ctypes.data, bd.ctypes.data) == 0
    assert (int(bi[0]), int(bd[0])) == (-1, 128)
    big[m - 1] = pc.with_bits(q[0], 7, 100)
    assert L.vio_pg_match(q.ctypes.data, 1, big.ctypes.data, m, bi.ctypes.data, bd.ctypes.data) == 0
    oi, od = O.o_match(q, big[:m])
    assert (int(bi[0]), int(bd[0])) == (m - 1, 7) == (int(oi[0]), int(od[0]))
    bi[:] = -9; bd[:] = -9
    assert L.vio_pg_match(q.ctypes.data, 1, big.ctypes.data, 0xFFFFF, bi.ctypes.data, bd.ctypes.data) == P.VIO_EINVAL
    assert bi[0] == -9 and bd[0] == -9


# ------------------------------------------------------------------------------------------------ vocabulary walk
def _hip_voc(PG, voc):
    return PG.Vocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["node_id"], voc["parent_id"], voc["weight"], voc["desc"],
                                     voc["word_node"], voc["word_id"])


def test_vocabulary_walk_few_descriptors_and_twin_siblings(PG):
    """one workgroup walks four descriptors: n = 1 .. 5 leave lanes of the last workgroup without one.  On the 70-way vocabulary whose
    siblings 3 and 67 (both lane 3's) are identical at the root and one level down, the twin's descriptor -- exact and with 5 bits
    toggled -- reaches child 3's word: the first child with the smallest distance."""
    voc, d_root3, d_leaf3, leaf3 = pc.twin_vocabulary()
    word3 = int(voc["word_id"][list(voc["word_node"]).index(leaf3)])
    o, h = bow_util.OracleVoc(voc), _hip_voc(PG, voc)
    feats = np.concatenate([np.array([d_leaf3, pc.with_bits(d_leaf3, 5, 17), pc.with_bits(d_leaf3, 5, 200), d_root3], np.uint64),
                            bow_util.view_of(bow_util.place_descriptors(voc, 1, 40), 2, noise_bits=20, extra=8)])
    for n in (1, 2, 3, 4, 5, len(feats)):
        w, wt = h.transform(feats[:n])
        wo, wto = o.transform(feats[:n])
        assert np.array_equal(w, wo) and np.array_equal(wt, wto), (n, w.tolist(), wo.tolist())
        for f, wi, wti in zip(feats[:n], w, wt):
            assert bow_util.reference_walk(voc, f) == (int(wi), float(wti)), n
    w, _ = h.transform(feats[:3])
    assert w.tolist() == [word3] * 3
    assert len(h.transform(feats[:0])[0]) == 0
    o.close(); h.close()
    # a narrow, deep tree: the same counts
    voc = bow_util.make_vocabulary(10, 4, 17)
    o, h = bow_util.OracleVoc(voc), _hip_voc(PG, voc)
    feats = bow_util.view_of(bow_util.place_descriptors(voc, 3, 8), 4, noise_bits=20, extra=2)
    for n in (1, 2, 3, 4, 5):
        w, wt = h.transform(feats[:n])
        wo, wto = o.transform(feats[:n])
        assert np.array_equal(w, wo) and np.array_equal(wt, wto), n
    o.close(); h.close()


# ------------------------------------------------------------------------------------------------ argument checks
def test_describe_refuses_sizes_and_thresholds_outside_its_range(P, L):
    """16 .. 4095 each way, thresholds 1 .. 254: anything else is VIO_EINVAL from the host check, before any launch (return codes only;
    the buffers are as large as the refused call would need)"""
    img = np.zeros(4096 * 4096, np.uint8)
    for (W, H) in ((15, 16), (16, 15), (4096, 16), (16, 4096), (15, 4096)):
        rc, _, kxy, kd, kn = _describe_raw(L, P.canonical_config(width=W, height=H), img, NONE, 20, 4, 4)
        assert rc == P.VIO_EINVAL, (W, H, rc)
        assert (kxy == -7.0).all()
    for thr in (0, 255, -1):
        rc, _, kxy, kd, kn = _describe_raw(L, P.canonical_config(width=16, height=16), img, NONE, thr, 4, 4)
        assert rc == P.VIO_EINVAL, (thr, rc)
    out = np.zeros(16 * 16, np.uint8)
    assert L.vio_pg_stage_blur(img.ctypes.data, 15, 16, out.ctypes.data) == P.VIO_EINVAL
    assert _describe_raw(L, P.canonical_config(width=16, height=16), img, NONE, 1, 4, 4)[0] >= 0     # the smallest legal call goes through
