"""Pins the inputs of tests/test_gpu_posegraph_edges.py with the oracle alone (oracle/posegraph.cpp, oracle/bow.cpp), so that the GPU
comparisons cannot pass vacuously: the oracle equals the plain-numpy definitions of tests/posegraph_cases.py at every size, the images
really give keypoints (and really give none where the empty list is meant), the truncation input really has 842 keypoints, every class of
window point is present, and the constructed Hamming and vocabulary cases really have the answers they were built for.  Every count is a
property of the deterministic inputs, asserted with the oracle's figure on an x86-64 CPU."""
import numpy as np
import pytest

import bow_util
import posegraph_cases as pc
import test_oracle_posegraph_cpu as O

# keypoints of ovio_pg_describe per (kind, threshold), one row per size of pc.SIZES
COUNTS = {
    (16, 16): dict(noise=(12, 9, 0), binary=(3, 3, 3), texture=(3, 1, 0)),
    (17, 23): dict(noise=(23, 23, 0), binary=(4, 4, 4), texture=(8, 8, 0)),
    (63, 17): dict(noise=(69, 67, 0), binary=(9, 9, 9), texture=(21, 13, 0)),
    (65, 33): dict(noise=(168, 159, 0), binary=(13, 13, 13), texture=(51, 34, 0)),
    (70, 22): dict(noise=(108, 101, 0), binary=(15, 15, 15), texture=(26, 21, 0)),
    (71, 22): dict(noise=(118, 106, 0), binary=(15, 15, 15), texture=(36, 21, 0)),
    (129, 31): dict(noise=(327, 303, 0), binary=(21, 21, 21), texture=(104, 63, 0)),
    (200, 50): dict(noise=(913, 842, 0), binary=(56, 56, 56), texture=(255, 173, 0)),
    (848, 480): dict(noise=(42541, 39947, 0), binary=(2593, 2593, 2593), texture=(11061, 7473, 0)),
    (1280, 720): dict(noise=(96617, 90678, 0), binary=(5629, 5629, 5629), texture=(25190, 17018, 0)),
    (4095, 16): dict(noise=(4715, 4323, 0), binary=(343, 343, 343), texture=(1544, 943, 0)),
}


def _blur(img):
    H, W = img.shape
    out = np.zeros_like(img)
    O.olib().ovio_pg_blur(img.ctypes.data, W, H, out.ctypes.data)
    return out


def test_the_cases_are_the_ones_the_kernels_were_read_for():
    """the chunk arithmetic in the comments of pc.SIZES, the reach of the pattern, and the vectorised FAST definition against the
    pixel-by-pixel one of test_oracle_kat on the small sizes"""
    chunks = {s: ((s[0] - 6) * (s[1] - 6) + 63) // 64 for s in pc.SIZES}
    assert chunks[(16, 16)] == 2 and (70 - 6) * (22 - 6) == 1024 and chunks[(70, 22)] == 16 and chunks[(71, 22)] == 17
    assert all(16 <= W <= 4095 and 16 <= H <= 4095 for W, H in pc.SIZES)
    assert any(W % 64 and H % 16 for W, H in pc.SIZES) and (1280 % 64, 720 % 16) == (0, 0) and 848 % 64 == 16
    pat = pc.pattern()
    assert np.array_equal(pat, O.pattern()) and np.abs(pat).max() == pc.REACH
    assert [s for s in pc.SIZES if pc.has_interior(*s)] == [(200, 50), (848, 480), (1280, 720)]
    assert pc.SMALL == [s for s in pc.SIZES if s not in ((848, 480), (1280, 720), (4095, 16))]
    for (W, H) in ((16, 16), (17, 23), (63, 17)):
        for kind in pc.KINDS:
            for thr in pc.THRESHOLDS:
                assert np.array_equal(pc.fast_keypoints_def(pc.image(kind, W, H), thr), pc.fast_keypoints_loop(pc.image(kind, W, H), thr)), (W, H, kind, thr)


@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_oracle_equals_the_definitions(P, size):
    """ovio_pg_blur == blur_def; the keypoints of ovio_pg_describe at thresholds 1, 20 and 254 equal fast_keypoints_def in value and
    order; window and keypoint descriptors equal brief_def; kp_norm equals lift_def -- bit for bit: numpy's float64 reproduces the
    oracle's eight iterations exactly (no last-bit difference anywhere, so the one-ulp allowance is not used), NaN payloads included on
    this CPU (pc.same_floats does not insist on those)."""
    W, H = size
    cfg = P.canonical_config(width=W, height=H)
    uv, pat = pc.all_window_points(W, H), pc.pattern()
    assert not np.isnan(uv).any()
    for kind in pc.KINDS:
        img = pc.image(kind, W, H)
        blur = _blur(img)
        assert np.array_equal(blur, pc.blur_def(img)), kind
        counts = []
        for thr in pc.THRESHOLDS:
            wd, kxy, kd, kn = O.o_describe(cfg, img, uv, pat, thr, cap=100000)
            assert np.array_equal(kxy, pc.fast_keypoints_def(img, thr)), (kind, thr)
            assert len(kxy) < 2 or (np.diff(kxy[:, 1] * W + kxy[:, 0]) > 0).all()
            assert np.array_equal(wd, pc.brief_def(blur, uv, pat)), (kind, thr)
            assert np.array_equal(kd, pc.brief_def(blur, kxy, pat)), (kind, thr)
            assert pc.same_floats(kn, pc.lift_def(cfg, kxy)), (kind, thr)
            counts.append(len(kxy))
        assert tuple(counts) == COUNTS[size][kind], (kind, counts)


def test_the_images_give_what_they_are_for():
    """noise: keypoints at threshold 20 everywhere (fewest: 9 at 16 x 16); binary: the same non-zero count at thresholds 1, 20 and 254
    (every corner score is 254, the top of the uint8 score; fewest: 3 at 16 x 16); noise and texture: none at 254, the empty-list path;
    200 x 50 noise at 20: the 842 keypoints of the truncation test; 848 x 480 noise: more than the 8192 posegraph.describe starts with"""
    assert set(COUNTS) == set(pc.SIZES)
    assert min(c["noise"][1] for c in COUNTS.values()) == 9 == COUNTS[(16, 16)]["noise"][1]
    assert all(c["binary"][0] == c["binary"][1] == c["binary"][2] > 0 for c in COUNTS.values())
    assert min(c["binary"][0] for c in COUNTS.values()) == 3 == COUNTS[(16, 16)]["binary"][0]
    assert all(c["noise"][2] == 0 and c["texture"][2] == 0 for c in COUNTS.values())
    assert COUNTS[pc.TRUNCATION_SIZE]["noise"][pc.THRESHOLDS.index(pc.TRUNCATION_THRESHOLD)] == pc.TRUNCATION_TOTAL == 842
    assert COUNTS[(848, 480)]["noise"][1] > 8192
    for (W, H) in ((16, 16), (200, 50)):     # the binary image's scores: 0 or 254, nothing between
        sc = pc.fast_scores_def(pc.image("binary", W, H), 1)
        assert set(np.unique(sc).tolist()) == {0, 254}
    flat = pc.image("flat", 200, 50)
    assert np.array_equal(_blur(flat), flat) and len(pc.fast_keypoints_def(flat, 1)) == 0


@pytest.mark.parametrize("size", pc.SIZES, ids=pc.size_id)
def test_every_class_of_window_point_is_present(size):
    W, H = size
    pts = pc.window_points(W, H)
    pat = pc.pattern().reshape(4, 256).astype(np.float32)

    def pairs_inside(p):
        x1, y1, x2, y2 = ((np.float32(p[k % 2]) + pat[k]).astype(np.int32) for k in range(4))
        return int(((x1 >= 0) & (x1 < W) & (y1 >= 0) & (y1 < H) & (x2 >= 0) & (x2 < W) & (y2 >= 0) & (y2 < H)).sum())

    assert ("interior" in pts) == pc.has_interior(W, H)
    for name, p in pts.items():
        assert len(p) > 0 and p.dtype == np.float32 and not np.isnan(p).any(), name
    if "interior" in pts:
        assert all(pairs_inside(p) == 256 for p in pts["interior"])
        assert all(pairs_inside(p) == 256 for p in pc.to_interior(pts["near_border"], W, H))
    nb = pts["near_border"]
    assert ((nb >= 0).all(1) & (nb[:, 0] <= W - 1) & (nb[:, 1] <= H - 1)).all()
    for side in (nb[:, 0] < pc.REACH, nb[:, 0] > W - 1 - pc.REACH, nb[:, 1] < pc.REACH, nb[:, 1] > H - 1 - pc.REACH):
        assert side.sum() >= 4
    assert all(pairs_inside(p) < 256 for p in nb)
    by = pts["beyond"]
    outside = (by[:, 0] < 0) | (by[:, 0] > W - 1) | (by[:, 1] < 0) | (by[:, 1] > H - 1)
    assert outside.all() and by[:, 0].min() == -3 and by[:, 0].max() == W + 2 and by[:, 1].min() == -3 and by[:, 1].max() == H + 2
    for side in (by[:, 0] < 0, by[:, 0] > W - 1, by[:, 1] < 0, by[:, 1] > H - 1):
        assert side.sum() >= 2
    tr = pts["truncation"]
    assert (tr[:, 0] == -0.5).any() and (tr[:, 0] == W - 0.5).any() and (tr[:, 1] == -0.5).any() and (tr[:, 1] == H - 0.5).any()
    assert (tr == np.floor(tr)).all(1).sum() >= 3
    # (int) truncates toward zero: the pattern has pairs with a zero offset, and for those -0.5 + 0 samples column 0 (a floor would make
    # it -1, outside), so a point at x = -0.5 keeps pairs that one at x = -1 loses
    assert (pat[0] == 0).any() and (pat[2] == 0).any() and (np.float32(-0.5) + pat[0][pat[0] == 0]).astype(np.int32).tolist()[0] == 0
    y = np.float32(H * 0.5 + 0.25)
    assert pairs_inside((-0.5, y)) > pairs_inside((-1.0, y))
    if pc.has_interior(W, H):
        img = pc.image("noise", W, H)
        blur = _blur(img)
        near = pc.popcount(pc.brief_def(blur, nb, pc.pattern()))
        moved = pc.popcount(pc.brief_def(blur, pc.to_interior(nb, W, H), pc.pattern()))
        assert (near < moved).sum() >= 1 and (near < moved).sum() >= len(nb) // 2, (near.tolist(), moved.tolist())


def test_constructed_hamming_cases():
    """the all-zero query against one candidate on both sides of the acceptance (80) and of the floor (128), and the two tie sets"""
    assert pc.popcount(pc.with_bits(pc.ZERO, 79, 100)) == 79 and pc.popcount(pc.with_bits(pc.with_bits(pc.ZERO, 256), 256)) == 0
    assert pc.with_bits(pc.ZERO, 3, 63).tolist() == [1 << 63, 3, 0, 0]
    q = pc.ZERO.reshape(1, 4)
    for dist, want in pc.SINGLE_CASES:
        b = pc.single_candidate(dist)
        assert pc.hamming_def(q, b)[0, 0] == dist
        for bi, bd in (O.o_match(q, b), pc.match_def(q, b)):
            assert (int(bi[0]), int(bd[0])) == want, (dist, bi, bd)
    assert [w for _, w in pc.SINGLE_CASES] == [(0, 0), (0, 79), (-1, 80), (-1, 127), (-1, 128), (-1, 128)]
    for bi, bd in (O.o_match(q, np.zeros((0, 4), np.uint64)), pc.match_def(q, np.zeros((0, 4), np.uint64))):
        assert (int(bi[0]), int(bd[0])) == (-1, 128)
    b, want = pc.tie_case_lanes()
    d = pc.hamming_def(q, b)[0]
    assert want == (6, 10) and len(b) == 200 and np.flatnonzero(d == 10).tolist() == [6, 69, 70, 134] and (np.delete(d, [6, 69, 70, 134]) == 100).all()
    assert 70 % 64 == 134 % 64 == 6 and 69 % 64 == 5
    assert len(np.unique(b, axis=0)) == 200
    for bi, bd in (O.o_match(q, b), pc.match_def(q, b)):
        assert (int(bi[0]), int(bd[0])) == want
    b, want = pc.tie_case_later_lane()
    d = pc.hamming_def(q, b)[0]
    assert want == (11, 10) and np.flatnonzero(d == 10).tolist() == [11, 74] and 74 % 64 < 11 % 64
    for bi, bd in (O.o_match(q, b), pc.match_def(q, b)):
        assert (int(bi[0]), int(bd[0])) == want


def test_match_def_equals_the_oracle_on_real_descriptors(P):
    """keypoint descriptors of two shifted crops of one texture: real near-duplicates, m around the wavefront width"""
    W, H = 200, 50
    cfg = P.canonical_config(width=W, height=H)
    g0, g1 = pc.fc.texture_pair(W, H, 2, -1)
    none = np.zeros((0, 2), np.float32)
    a = O.o_describe(cfg, g1, none, pc.pattern(), 20)[2]
    b = O.o_describe(cfg, g0, none, pc.pattern(), 20)[2]
    assert len(a) > 65 and len(b) > 129
    for m in (0, 1, 63, 64, 65, 127, 128, 129, len(b)):
        bi, bd = O.o_match(a, b[:m])
        di, dd = pc.match_def(a, b[:m])
        assert np.array_equal(bi, di) and np.array_equal(bd, dd), m
        if m == 63:     # most partners are missing from the short list: rejections between 80 and 127 (natural descriptors never reach
            assert (bi == -1).sum() >= 20 and ((bd >= 80) & (bd < 128)).sum() >= 20, (bi.tolist(), bd.tolist())   # the floor of 128)
    assert (bi >= 0).sum() >= 20


def test_twin_vocabulary_walks_to_the_first_twin():
    """the (70, 2) vocabulary with siblings 3 and 67 identical at the root and one level down: the twin's descriptor, and the same with 5
    bits toggled, reach child 3's word -- in the oracle and in the pure-Python walk"""
    voc, d_root3, d_leaf3, leaf3 = pc.twin_vocabulary()
    word3 = int(voc["word_id"][list(voc["word_node"]).index(leaf3)])
    o = bow_util.OracleVoc(voc)
    assert o.info()[:2] == [70, 2]
    root_kids = voc["node_id"][voc["parent_id"] == 0]
    kids = voc["node_id"][voc["parent_id"] == root_kids[3]]
    assert np.array_equal(voc["desc"][root_kids[67] - 1], d_root3) and np.array_equal(voc["desc"][kids[67] - 1], d_leaf3) and kids[3] == leaf3
    queries = np.array([d_leaf3, pc.with_bits(d_leaf3, 5, 17), pc.with_bits(d_leaf3, 5, 200)], np.uint64)
    for f in queries:   # the ties are exact at both levels, and nothing else is as near
        dr = np.array([bow_util.hamming(f, voc["desc"][c - 1]) for c in root_kids])
        dk = np.array([bow_util.hamming(f, voc["desc"][c - 1]) for c in kids])
        assert dr[3] == dr[67] == dr.min() and (dr == dr.min()).sum() == 2
        assert dk[3] == dk[67] == dk.min() and (dk == dk.min()).sum() == 2
    w, wt = o.transform(queries)
    assert w.tolist() == [word3] * 3
    for f, wi, wti in zip(queries, w, wt):
        assert bow_util.reference_walk(voc, f) == (int(wi), float(wti))
    # the root twin's own descriptor stays in child 3's subtree as well
    w2, _ = o.transform(d_root3.reshape(1, 4))
    assert bow_util.reference_walk(voc, d_root3)[0] == int(w2[0])
    assert int(voc["word_node"][int(w2[0])]) in kids.tolist()
    o.close()
