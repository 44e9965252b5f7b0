"""Deterministic inputs and plain-numpy definitions for the pose-graph kernel edge tests (csrc/pg_kernels.hip, csrc/pg_bow.hip):
test_posegraph_edges_cpu.py pins them with the oracle alone, test_gpu_posegraph_edges.py runs the kernels on them.  No GPU, no oracle,
fixed seeds; the images are frontend_cases' at their default seeds.

Every definition is written from the operation's description (the comments of pg_kernels.hip, cv::GaussianBlur / cv::FAST / DVision::BRIEF /
KeyFrame::searchByBRIEFDes / PinholeCamera::liftProjective), not from the oracle's code, and is integer arithmetic apart from lift_def."""
import functools
import hashlib
import os

import numpy as np

import frontend_cases as fc
from test_oracle_kat import RING

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (W, H); the kernels work on 64 x 16 tiles, the non-maximum kernel splits the (W - 6)(H - 6) interior pixels into 64-pixel chunks that 16
# wavefronts share in contiguous ranges
SIZES = [(16, 16),       # smallest legal: 10 x 10 = 100 interior pixels, 2 chunks, 14 idle wavefronts
         (17, 23),       # 11 x 17 = 187: small, no tile alignment either way
         (63, 17),       # 57 x 11 = 627: one pixel short of a tile's width, one row into the second tile row
         (65, 33),       # 59 x 27 = 1593: one pixel into the second tile column and into the third tile row
         (70, 22),       # 64 x 16 = 1024: exactly 16 full chunks, one per wavefront
         (71, 22),       # 65 x 16 = 1040: 17 chunks, two per wavefront, wavefronts 9 .. 15 idle
         (129, 31),      # 123 x 25 = 3075: partial tiles both ways
         (200, 50),      # 194 x 44 = 8536: partial tiles both ways; the smallest size with interior window points
         (848, 480),     # 842 x 474: a supported production size, 13.25 tiles wide
         (1280, 720),    # 1274 x 714: the other one, 20 x 45 full tiles
         (4095, 16)]     # 4089 x 10 = 40890: the width limit
KINDS = ("noise", "binary", "texture")
THRESHOLDS = (1, 20, 254)
SMALL = [s for s in SIZES if s[0] * s[1] <= 200 * 50]   # where the GPU tests compare with the numpy definitions as well
TRUNCATION_SIZE, TRUNCATION_THRESHOLD, TRUNCATION_TOTAL = (200, 50), 20, 842   # the `pos < cap` test's input and its keypoint count


def size_id(s):
    return "%dx%d" % s


@functools.lru_cache(maxsize=None)
def image(kind, W, H):
    img = {"noise": fc.noise, "binary": fc.binary, "texture": fc.texture, "flat": fc.flat}[kind](W, H)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def pattern():
    """int32[1024] = x1 | y1 | x2 | y2 of tests/golden/brief_pattern.npz, as the C ABI takes it"""
    z = np.load(os.path.join(GOLD, "brief_pattern.npz"))
    p = np.ascontiguousarray(np.concatenate([z[k].astype(np.int32).reshape(-1) for k in ("x1", "y1", "x2", "y2")]))
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------------------------------------ definitions
BLUR_TAPS = [7, 17, 32, 46, 52, 46, 32, 17, 7]


def blur_def(img):
    """cv::GaussianBlur(9 x 9, sigma 2) on uint8: exp(-x^2 / (2 sigma^2)) normalised, 8 fractional bits per pass, REFLECT_101, one rounding
    at the end"""
    H, W = img.shape
    k = np.exp(-np.arange(-4, 5) ** 2 / 8.0)
    ki = np.rint(k / k.sum() * 256).astype(np.int64)
    assert ki.sum() == 256 and list(ki) == BLUR_TAPS
    pad = np.pad(img.astype(np.int64), 4, mode="reflect")
    h = sum(ki[i] * pad[:, i:i + W] for i in range(9))
    v = sum(ki[i] * h[i:i + H, :] for i in range(9))
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


_strength = {}   # (shape, digest of the pixels) -> _fast_strength, so that the thresholds of one image share the ring minima


def _fast_strength(img):
    """the largest t for which 9 contiguous ring pixels are all > v + t or all < v - t, per interior pixel (negative where none); the 16
    ring offsets as 16 shifted views, test_oracle_kat.fast_score_def's arithmetic on whole arrays"""
    key = (img.shape, hashlib.sha1(np.ascontiguousarray(img).tobytes()).digest())
    if key not in _strength:
        if len(_strength) >= 4:
            _strength.clear()
        _strength[key] = _fast_strength_uncached(img)
    return _strength[key]


def _fast_strength_uncached(img):
    H, W = img.shape
    img = img.astype(np.int16)
    v = img[3:H - 3, 3:W - 3]
    d = np.stack([img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - v for dx, dy in RING])
    best = np.full(v.shape, -256, np.int16)
    for e in (d, -d):
        e2 = np.concatenate([e, e[:8]])
        for s in range(16):
            best = np.maximum(best, e2[s:s + 9].min(0) - 1)
    return best


def fast_scores_def(img, thr):
    """score image of cv::FAST(thr): fast_score_def(img, x, y, thr) for every pixel at least 3 from the border, 0 elsewhere"""
    H, W = img.shape
    best = _fast_strength(img)
    sc = np.zeros((H, W), np.int16)
    sc[3:H - 3, 3:W - 3] = np.where(best >= thr, best, 0)
    return sc


def fast_keypoints_def(img, thr):
    """cv::FAST(image, thr, nonmaxSuppression = true): pixels whose score is non-zero and strictly greater than all eight neighbours'
    (border scores are 0), in row-major order, as float32 (x, y)"""
    H, W = img.shape
    sc = fast_scores_def(img, thr)
    c = sc[1:-1, 1:-1]
    mx = c > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dx, dy) != (1, 1):
                mx &= c > sc[dy:H - 2 + dy, dx:W - 2 + dx]
    yx = np.argwhere(mx) + 1                                     # argwhere is row-major
    return np.ascontiguousarray(yx[:, ::-1], np.float32)


def fast_keypoints_loop(img, thr):
    """the same, pixel by pixel through test_oracle_kat.fast_score_def (small images only): the check of the vectorised form"""
    from test_oracle_kat import fast_score_def
    H, W = img.shape
    sc = np.zeros((H, W), np.int32)
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            sc[y, x] = fast_score_def(img, x, y, thr)
    out = []
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            nb = sc[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if sc[y, x] and sc[y, x] > nb.max():
                out.append((x, y))
    return np.array(out, np.float32).reshape(-1, 2)


def brief_def(blur, xy, pat, chunk=4096):
    """DVision::BRIEF::compute on the blurred image: bit i of a point = I(p + (x1, y1)_i) < I(p + (x2, y2)_i) when both samples are inside
    the image, else 0.  The additions are float32, the conversion to int truncates toward zero.  Returns uint64[n][4], bit i in word
    i / 64 at position i % 64."""
    H, W = blur.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    pf = np.asarray(pat, np.int32).astype(np.float32).reshape(4, 256)
    out = np.zeros((len(xy), 4), np.uint64)
    for a in range(0, len(xy), chunk):
        p = xy[a:a + chunk]
        x1, y1 = (p[:, 0:1] + pf[0]).astype(np.int32), (p[:, 1:2] + pf[1]).astype(np.int32)      # float32 + float32, then truncation
        x2, y2 = (p[:, 0:1] + pf[2]).astype(np.int32), (p[:, 1:2] + pf[3]).astype(np.int32)
        inside = (x1 >= 0) & (x1 < W) & (y1 >= 0) & (y1 < H) & (x2 >= 0) & (x2 < W) & (y2 >= 0) & (y2 < H)
        i1 = blur[np.clip(y1, 0, H - 1), np.clip(x1, 0, W - 1)]
        i2 = blur[np.clip(y2, 0, H - 1), np.clip(x2, 0, W - 1)]
        bits = inside & (i1 < i2)
        out[a:a + chunk] = np.packbits(bits.reshape(len(p), 4, 64), axis=2, bitorder="little").view("<u8").reshape(len(p), 4)
    return out


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def popcount(d):
    """set bits of each descriptor of uint64[n][4]"""
    return _POP8[np.ascontiguousarray(d, np.uint64).reshape(-1, 4).view(np.uint8)].sum(1)


def hamming_def(a, b):
    """int32[n][m] Hamming distances of uint64[n][4] against uint64[m][4]"""
    a, b = np.ascontiguousarray(a, np.uint64).reshape(-1, 4), np.ascontiguousarray(b, np.uint64).reshape(-1, 4)
    out = np.zeros((len(a), len(b)), np.int32)
    for i in range(len(a)):
        out[i] = _POP8[(a[i][None, :] ^ b).view(np.uint8)].sum(1) if len(b) else 0
    return out


def match_def(a, b):
    """KeyFrame::searchByBRIEFDes: per descriptor of a the first candidate of b with the smallest Hamming distance below 128; the distance
    (128 if there is none), and the candidate's index if the distance is below 80, else -1"""
    d = hamming_def(a, b)
    n = len(d)
    if d.shape[1] == 0:
        return np.full(n, -1, np.int32), np.full(n, 128, np.int32)
    first, dmin = d.argmin(1), d.min(1)                           # argmin returns the first occurrence
    return np.where(dmin < 80, first, -1).astype(np.int32), np.minimum(dmin, 128).astype(np.int32)


def lift_def(cfg, xy):
    """PinholeCamera::liftProjective: m_d = K^-1 (u, v), then eight fixed-point iterations m_u = m_d - distortion(m_u) of the
    radial-tangential model (k1, k2, p1, p2), in float64; the result rounded to float32"""
    uv = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    k1, k2, p1, p2 = float(cfg.k1), float(cfg.k2), float(cfg.p1), float(cfg.p2)
    mx_d = (1.0 / cfg.fx) * uv[:, 0] + (-cfg.cx / cfg.fx)
    my_d = (1.0 / cfg.fy) * uv[:, 1] + (-cfg.cy / cfg.fy)

    def distortion(x, y):
        mx2, my2, mxy = x * x, y * y, x * y
        rho2 = mx2 + my2
        rad = k1 * rho2 + k2 * rho2 * rho2
        return x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)

    mx_u, my_u = mx_d, my_d
    with np.errstate(all="ignore"):   # far outside the lens' field of view the iteration diverges to inf and NaN, as the reference's does
        for _ in range(8):
            dx, dy = distortion(mx_u, my_u)
            mx_u, my_u = mx_d - dx, my_d - dy
        return np.ascontiguousarray(np.stack([mx_u, my_u], 1).astype(np.float32))


def same_floats(a, b):
    """float32 arrays equal bit for bit.  The one exception is the payload of a NaN: canonical_config's 640 x 480 intrinsics on a 1280 or
    4095 px wide image put most keypoints far outside the lens' field of view, where the eight iterations end in inf - inf.  IEEE 754
    leaves the sign and payload of that NaN to the implementation (x86 gives 0xFFC00000, other processors 0x7FC00000), so NaN equals NaN
    here; everything else, the infinities and the 1e37s on the way there included, must be the same bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def with_bits(d, k, start=0):
    """a copy of the descriptor d (uint64[4]) with the k consecutive bits start .. start + k - 1 toggled"""
    assert 0 <= k and 0 <= start and start + k <= 256
    out = np.array(d, np.uint64).reshape(4).copy()
    for b in range(start, start + k):
        out[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
    return out


# ------------------------------------------------------------------------------------------------ window points
# The pattern of tests/golden/brief_pattern.npz reaches REACH = 24 px in x and in y (test_posegraph_edges_cpu.py asserts it), so a point has
# all 256 pairs inside the image only if 24 <= x < W - 24 and 24 <= y < H - 24: the interior class exists for W, H >= 49, which among SIZES
# means from 200 x 50 up.  None of the points is NaN: the conversion of NaN to int is undefined in the reference and differs between host
# and device; it is not part of the contract.
REACH = 24


def has_interior(W, H):
    return W >= 2 * REACH + 1 and H >= 2 * REACH + 1


def to_interior(p, W, H):
    """the points moved the shortest way into the region where all 256 pairs are inside"""
    p = np.asarray(p, np.float32).reshape(-1, 2)
    return np.ascontiguousarray(np.stack([np.clip(p[:, 0], REACH, W - 1 - REACH), np.clip(p[:, 1], REACH, H - 1 - REACH)], 1), np.float32)


def window_points(W, H):
    """{class: float32[n][2]} -- interior (where it exists), near each of the four borders, up to 3 px beyond each border, and the values
    on which truncation toward zero matters (-0.5 samples column 0, W - 0.5 samples column W - 1) plus integers"""
    cx, cy = np.float32(W * 0.5 + 0.25), np.float32(H * 0.5 + 0.25)
    out = {}
    if has_interior(W, H):
        fx, fy = W - 1 - 2 * REACH, H - 1 - 2 * REACH
        out["interior"] = [(REACH + f * fx + e, REACH + g * fy + e2) for f, g, e, e2 in
                           ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (0.5, 0.5, 0.3, 0.7), (0.25, 1.0, 0.6, 0.9), (1.0, 0.0, 0.9, 0.2))]
    inset = [0.0, 2.6, min(11.3, W - 1.0, H - 1.0), min(REACH - 4.0, W - 1.0, H - 1.0)]   # (upwards the pattern reaches 21 and 23 px only)
    out["near_border"] = ([(d, cy) for d in inset] + [(W - 1 - d, cy) for d in inset] + [(cx, d) for d in inset] + [(cx, H - 1 - d) for d in inset] +
                          [(1.4, 1.7), (W - 2.4, 1.2), (1.9, H - 2.6), (W - 2.1, H - 1.3)])
    out["beyond"] = [(-3.0, cy), (-1.5, cy), (W + 2.0, cy), (W + 0.5, cy), (cx, -3.0), (cx, -1.25), (cx, H + 2.0), (cx, H + 0.75),
                     (-3.0, -3.0), (W + 2.0, H + 2.0), (-2.0, H + 1.0), (W + 1.0, -2.0)]
    out["truncation"] = [(-0.5, cy), (W - 0.5, cy), (cx, -0.5), (cx, H - 0.5), (-0.5, -0.5), (W - 0.5, H - 0.5), (-0.5, H - 0.5), (W - 0.5, -0.5),
                         (0.0, 0.0), (W - 1.0, H - 1.0), (float(W // 2), float(H // 2)), (float(W), float(H)), (-1.0, -1.0)]
    return {k: np.ascontiguousarray(np.array(v, np.float64), np.float32).reshape(-1, 2) for k, v in out.items()}


def all_window_points(W, H):
    return np.ascontiguousarray(np.vstack(list(window_points(W, H).values())), np.float32)


# ------------------------------------------------------------------------------------------------ constructed Hamming cases
ZERO = np.zeros(4, np.uint64)   # the query of every constructed case

# a single candidate at this distance from the all-zero query -> (index, distance): accepted below 80, the distance floored at 128
SINGLE_CASES = [(0, (0, 0)), (79, (0, 79)), (80, (-1, 80)), (127, (-1, 127)), (128, (-1, 128)), (256, (-1, 128))]


def single_candidate(dist):
    return with_bits(ZERO, dist, 0).reshape(1, 4)


def _background():
    """200 different candidates at distance 100 from the all-zero query: 99 consecutive bits from j % 100 and bit 200 + j / 100"""
    return np.array([with_bits(with_bits(ZERO, 99, j % 100), 1, 200 + j // 100) for j in range(200)], np.uint64)


def tie_case_lanes():
    """200 candidates at distance 100 (all different), distance 10 planted at indices 70, 6, 134 and 69 in this order of construction.
    The first smallest is index 6.  On the device candidate j is lane j % 64's: 70 and 134 are in lane 6 with 6 itself, 69 is in lane 5.
    Returns (candidates, (expected index, expected distance))."""
    b = _background()
    for q, j in enumerate((70, 6, 134, 69)):
        b[j] = with_bits(ZERO, 10, 20 * q)
    return np.ascontiguousarray(b), (6, 10)


def tie_case_later_lane(k=10):
    """200 candidates at distance 100, the minimum (distance 10) only at 64 + k (lane k) and k + 1 (lane k + 1): the later lane holds the
    smaller index, which is the answer"""
    b = _background()
    b[64 + k] = with_bits(ZERO, 10, 3)
    b[k + 1] = with_bits(ZERO, 10, 77)
    return np.ascontiguousarray(b), (k + 1, 10)


# ------------------------------------------------------------------------------------------------ vocabulary with identical siblings
def twin_vocabulary():
    """bow_util.make_vocabulary(70, 2, ...): 70-way nodes, wider than a wavefront, so that children 3 and 67 of a node are both lane 3's.
    Sibling 67 of the root gets sibling 3's descriptor, and sibling 67 among child 3's children gets that node's child 3's descriptor.
    Returns (voc, root child 3's descriptor, its child 3's descriptor, the node id of that grandchild)."""
    import bow_util
    voc = bow_util.make_vocabulary(70, 2, 77)
    voc = dict(voc, desc=voc["desc"].copy())
    nid, pid = voc["node_id"], voc["parent_id"]
    root_kids = nid[pid == 0]
    assert len(root_kids) == 70
    voc["desc"][root_kids[67] - 1] = voc["desc"][root_kids[3] - 1]
    kids = nid[pid == root_kids[3]]
    assert len(kids) == 70
    voc["desc"][kids[67] - 1] = voc["desc"][kids[3] - 1]
    return voc, voc["desc"][root_kids[3] - 1].copy(), voc["desc"][kids[3] - 1].copy(), int(kids[3])
