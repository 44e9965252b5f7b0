"""Definitions behind the device pose solvers, in high precision (mpmath, 50 digits), and the restatement of solveRelativeR extended to
correspondences that its RANSAC rejects.

exp_mp / dexp_mp / log_mp: the exponential map of SO(3), its derivative with respect to the rotation vector in closed form (checked
against a central difference in mpmath itself by tests/test_pose_ref_cpu.py) and the logarithm with theta in [0, pi].

solve_relative_r: excalib_ref.solve_relative_r with an inlier mask (run8point on the inliers, the four votes over ALL correspondences) and
the details that vio_stage_relative_r_detail reports; ransac_mask gets the mask from the oracle's own sampler."""
import ctypes as C

import mpmath as mp
import numpy as np

import excalib_ref as X

mp.mp.dps = 50


def _skew(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def exp_mp(r):
    """R = exp(skew(r)), 3 x 3 mp.matrix; r: three numbers (doubles are taken exactly)"""
    r = [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in r]
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    th = mp.sqrt(th2)
    K = _skew(r)
    if th == 0:
        return mp.eye(3)
    a = mp.sin(th) / th
    b = (1 - mp.cos(th)) / th2
    return mp.eye(3) + a * K + b * (K * K)


def dexp_mp(r):
    """[dR/dr_0, dR/dr_1, dR/dr_2] by differentiating R = I + a K + b K^2, a = sin(th)/th, b = (1 - cos th)/th^2:
    dR/dr_i = a' (r_i/th) K + a G_i + b' (r_i/th) K^2 + b (G_i K + K G_i); at th = 0 the generators G_i"""
    r = [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in r]
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    G = [_skew([mp.mpf(i == 0), mp.mpf(i == 1), mp.mpf(i == 2)]) for i in range(3)]
    if th2 == 0:
        return G
    th = mp.sqrt(th2)
    K = _skew(r)
    K2 = K * K
    s, c = mp.sin(th), mp.cos(th)
    a, b = s / th, (1 - c) / th2
    da = (c * th - s) / th2            # d a / d th
    db = (s * th - 2 * (1 - c)) / (th2 * th)
    return [da * (r[i] / th) * K + a * G[i] + db * (r[i] / th) * K2 + b * (G[i] * K + K * G[i]) for i in range(3)]


def log_mp(R):
    """rotation vector of a rotation matrix (mp.matrix or array of doubles), theta in [0, pi]; at theta = pi the axis sign that makes the
    first non-zero component positive"""
    R = mp.matrix([[mp.mpf(float(R[i, j])) if not isinstance(R[i, j], mp.mpf) else R[i, j] for j in range(3)] for i in range(3)])
    v = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) / 2
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = mp.atan2(s, c)
    if s > mp.mpf("1e-20"):
        return [th / (2 * s) * x for x in v]
    if c > 0:
        return [x / 2 for x in v]
    # theta = pi (to 1e-20): R = 2 k k^T - I
    B = (R + mp.eye(3)) / 2
    i = max(range(3), key=lambda q: B[q, q])
    k = [B[i, j] / mp.sqrt(B[i, i]) for j in range(3)]
    sg = next((1 if x > 0 else -1) for x in k if x != 0)
    return [sg * th * x for x in k]


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def max_abs_diff(M, A):
    """max |M - A| evaluated in mpmath: M an mp.matrix, A a 3 x 3 array of doubles"""
    return float(max(abs(M[i, j] - mp.mpf(float(A[i, j]))) for i in range(3) for j in range(3)))


# ------------------------------------------------------------------------------------------------------------- solveRelativeR
def ransac_mask(orc, P, corres):
    """the inlier mask of cv::findFundamentalMat(FM_RANSAC, 3.0, 0.99) as ex_relative_r runs it (ransac_block(9.0, 1000, ...) on the
    float-rounded coordinates): the oracle's sampler with focal_length = 1, width = height = 0 (no lifting through pixels), f_threshold = 3,
    ransac_max_iters = 1000"""
    corres = np.asarray(corres, np.float64).reshape(-1, 6)
    cfg = P.canonical_config()
    cfg.focal_length, cfg.width, cfg.height, cfg.f_threshold, cfg.ransac_max_iters = 1.0, 0, 0, 3.0, 1000
    p1 = np.ascontiguousarray(corres[:, 0:2], np.float32)
    p2 = np.ascontiguousarray(corres[:, 3:5], np.float32)
    st = np.zeros(len(corres), np.uint8)
    orc.ovio_ransac(C.byref(cfg), len(corres), p1.ctypes.data, p2.ctypes.data, st.ctypes.data)
    return st.astype(bool)


def solve_relative_r(corres, mask=None):
    """(R, detail): detail = dict(found, inliers, cnt (the four votes of (R1, t) (R1, -t) (R2, t) (R2, -t)), win (1 / 2), flip, F22 (the
    entry F(2,2) before the normalisation), R1, R2).  mask None: every correspondence an inlier (excalib_ref.solve_relative_r)."""
    corres = np.asarray(corres, np.float64).reshape(-1, 6)
    none = dict(found=0, inliers=0, cnt=(0, 0, 0, 0), win=0, flip=0, F22=None)
    if len(corres) < 9:
        return np.eye(3), none
    p1 = corres[:, 0:2].astype(np.float32).astype(np.float64)
    p2 = corres[:, 3:5].astype(np.float32).astype(np.float64)
    mask = np.ones(len(corres), bool) if mask is None else np.asarray(mask, bool)
    ninl = int(mask.sum())
    if ninl < 8:
        return np.eye(3), dict(none, inliers=ninl)
    F, F22 = run8point_raw(p1[mask], p2[mask])
    if F is None:
        return np.eye(3), dict(none, inliers=ninl)
    R1, R2, t, flip = decompose_e(F)
    cnt = (X.front_count(p1, p2, R1, t), X.front_count(p1, p2, R1, -t), X.front_count(p1, p2, R2, t), X.front_count(p1, p2, R2, -t))
    win = 1 if max(cnt[0], cnt[1]) > max(cnt[2], cnt[3]) else 2
    R = (R1 if win == 1 else R2).T.copy()
    return R, dict(found=1, inliers=ninl, cnt=cnt, win=win, flip=flip, F22=F22, R1=R1.T.copy(), R2=R2.T.copy())


def run8point_raw(p1, p2):
    """excalib_ref.run8point, also returning F(2,2) as it stands before the `> FLT_EPSILON` normalisation"""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, c2 = p1.mean(0), p2.mean(0)
    s1, s2 = np.linalg.norm(p1 - c1, axis=1).mean(), np.linalg.norm(p2 - c2, axis=1).mean()
    if s1 < X.FLT_EPS or s2 < X.FLT_EPS:
        return None, None
    s1, s2 = np.sqrt(2.0) / s1, np.sqrt(2.0) / s2
    x1, y1 = (p1[:, 0] - c1[0]) * s1, (p1[:, 1] - c1[1]) * s1
    x2, y2 = (p2[:, 0] - c2[0]) * s2, (p2[:, 1] - c2[1]) * s2
    r = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], 1)
    w, V = X._eig_desc(r.T @ r)
    i = next((k for k in range(9) if abs(w[k]) < X.DBL_EPS), 9)
    if i < 8:
        return None, None
    F0 = X._canon(V[:, 8]).reshape(3, 3)
    _, V3 = X._eig_desc(F0.T @ F0)
    v3 = X._canon(V3[:, 2])
    F0 = F0 - np.outer(F0 @ v3, v3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1.0]])
    F = T2.T @ F0 @ T1
    f22 = float(F[2, 2])
    if abs(f22) > X.FLT_EPS:
        F = F / f22
    return F, f22


def decompose_e(E):
    """excalib_ref.decompose_e, also returning whether the det(R1) = -1 sign flip fired"""
    _, V = X._eig_desc(E.T @ E)
    v0, v2 = X._canon(V[:, 0]), X._canon(V[:, 2])
    v1 = np.cross(v2, v0)
    u0, u1 = E @ v0, E @ v1
    u0, u1 = u0 / np.linalg.norm(u0), u1 / np.linalg.norm(u1)
    u2 = np.cross(u0, u1)
    R1 = -np.outer(u0, v1) + np.outer(u1, v0) + np.outer(u2, v2)
    R2 = np.outer(u0, v1) - np.outer(u1, v0) + np.outer(u2, v2)
    t = u2
    flip = int(np.linalg.det(R1) + 1.0 < 1e-9)
    if flip:
        R1, R2, t = -R1, -R2, -t
    return R1, R2, t, flip
