"""estimate_extrinsic = 2: a float64 numpy restatement of InitialEXRotation (vins_estimator/src/initial/initial_ex_rotation.cpp) and a
test-side scene generator with strong rotation about all three axes.

Restatement: Eigen's matrix -> quaternion rule, cv::findFundamentalMat as DESIGN.md deviation 17 builds it (with the 3.0 threshold in
normalised units every correspondence is an inlier of the first RANSAC hypothesis, so F is the Hartley-normalised 8-point solution on all of
them), decomposeE and the four triangulation votes with the sign convention of be_excalib.h (canonical eigenvector signs, right-handed V),
the Huber-weighted averaging through a Jacobi-free FP64 eigen-solve of A^T A (deviation 18).

Generator: body pose R_wb(t), p_wb(t) analytic; IMU at 200 Hz by finite differences (as synth_host.cpp does); a fixed landmark set seen
through a known extrinsic (ric_true, tic_true) as xyz_uv_vel feature maps; a depth image with the true depth at every feature pixel."""
import numpy as np

FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------------------- rotations
def R2q(R):
    """Eigen Quaternion(Matrix3): (w, x, y, z)"""
    m = np.asarray(R, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k, j] - m[j, k]) * t
    q[1 + j] = (m[j, i] + m[i, j]) * t
    q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def q2R(q):
    """Eigen toRotationMatrix of (w, x, y, z), no normalisation"""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def rot_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra).T @ np.asarray(Rb)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def rodrigues(v):
    th = float(np.linalg.norm(v))
    if th < 1e-300:
        return np.eye(3)
    k = np.asarray(v, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


# ------------------------------------------------------------------------------------------------------------- restatement
def _canon(v):
    v = np.asarray(v, np.float64)
    i = int(np.argmax(np.abs(v)))
    return -v if v[i] < 0 else v.copy()


def _eig_desc(M):
    w, V = np.linalg.eigh(np.asarray(M, np.float64))
    o = np.argsort(-w, kind="stable")
    return w[o], V[:, o]


def run8point(p1, p2):
    """cv::findFundamentalMat's run8Point (Hartley normalisation, 9 x 9 normal matrix, rank-2 projection, F(2,2) = 1); None = no model"""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, c2 = p1.mean(0), p2.mean(0)
    s1, s2 = np.linalg.norm(p1 - c1, axis=1).mean(), np.linalg.norm(p2 - c2, axis=1).mean()
    if s1 < FLT_EPS or s2 < FLT_EPS:
        return None
    s1, s2 = np.sqrt(2.0) / s1, np.sqrt(2.0) / s2
    x1, y1 = (p1[:, 0] - c1[0]) * s1, (p1[:, 1] - c1[1]) * s1
    x2, y2 = (p2[:, 0] - c2[0]) * s2, (p2[:, 1] - c2[1]) * s2
    r = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], 1)
    w, V = _eig_desc(r.T @ r)
    i = next((k for k in range(9) if abs(w[k]) < DBL_EPS), 9)
    if i < 8:
        return None
    F0 = _canon(V[:, 8]).reshape(3, 3)
    _, V3 = _eig_desc(F0.T @ F0)
    v3 = _canon(V3[:, 2])
    F0 = F0 - np.outer(F0 @ v3, v3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1.0]])
    F = T2.T @ F0 @ T1
    if abs(F[2, 2]) > FLT_EPS:
        F = F / F[2, 2]
    return F


def decompose_e(E):
    """(R1, R2, t) with be_excalib.h's convention"""
    _, V = _eig_desc(E.T @ E)
    v0, v2 = _canon(V[:, 0]), _canon(V[:, 2])
    v1 = np.cross(v2, v0)
    u0, u1 = E @ v0, E @ v1
    u0, u1 = u0 / np.linalg.norm(u0), u1 / np.linalg.norm(u1)
    u2 = np.cross(u0, u1)
    R1 = -np.outer(u0, v1) + np.outer(u1, v0) + np.outer(u2, v2)
    R2 = np.outer(u0, v1) - np.outer(u1, v0) + np.outer(u2, v2)
    t = u2
    if np.linalg.det(R1) + 1.0 < 1e-9:
        R1, R2, t = -R1, -R2, -t
    return R1, R2, t


def front_count(p1, p2, R, t):
    """testTriangulation's count: P = [I | 0], P1 = [R | t] in float32, DLT per point, in front of both cameras"""
    P1 = np.hstack([R, t.reshape(3, 1)]).astype(np.float32).astype(np.float64)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    n = 0
    for (x1, y1), (x2, y2) in zip(p1, p2):
        A = np.stack([x1 * P0[2] - P0[0], y1 * P0[2] - P0[1], x2 * P1[2] - P1[0], y2 * P1[2] - P1[1]])
        _, V = _eig_desc(A.T @ A)
        X = V[:, 3]
        if X[2] / X[3] > 0 and (P1[2] @ X) / X[3] > 0:
            n += 1
    return n


def solve_relative_r(corres, detail=False):
    """solveRelativeR(corres): corres [n][6] = (x, y, z) of frame l, (x, y, z) of frame r.  detail=True also returns which of R1 / R2 won."""
    corres = np.asarray(corres, np.float64).reshape(-1, 6)
    if len(corres) < 9:
        return (np.eye(3), None) if detail else np.eye(3)
    p1 = corres[:, 0:2].astype(np.float32).astype(np.float64)
    p2 = corres[:, 3:5].astype(np.float32).astype(np.float64)
    F = run8point(p1, p2)
    if F is None:
        return (np.eye(3), None) if detail else np.eye(3)
    R1, R2, t = decompose_e(F)
    r1 = max(front_count(p1, p2, R1, t), front_count(p1, p2, R1, -t))
    r2 = max(front_count(p1, p2, R2, t), front_count(p1, p2, R2, -t))
    win = 1 if r1 > r2 else 2
    R = (R1 if win == 1 else R2).T.copy()
    return (R, dict(win=win, R1=R1.T.copy(), R2=R2.T.copy(), votes=(r1, r2), F=F)) if detail else R


def LmR(qc, qi):
    w, q = qc[0], np.asarray(qc[1:])
    L = np.zeros((4, 4))
    L[:3, :3] = w * np.eye(3) + np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
    L[:3, 3], L[3, :3], L[3, 3] = q, -q, w
    w, q = qi[0], np.asarray(qi[1:])
    R = np.zeros((4, 4))
    R[:3, :3] = w * np.eye(3) - np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
    R[:3, 3], R[3, :3], R[3, 3] = q, -q, w
    return L - R


def average(history, calls, window):
    """the averaging step of CalibrationExRotation over history [n][3][4] = q(Rc), q(Rimu), q(Rc_g): (ric, singular values, success)"""
    AtA = np.zeros((4, 4))
    for qc, qi, qg in np.asarray(history, np.float64).reshape(-1, 3, 4):
        d = qmul(qc, qg * np.array([1, -1, -1, -1]))
        ang = np.degrees(2.0 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0])))
        hub = 5.0 / ang if ang > 5.0 else 1.0
        M = hub * LmR(qc, qi)
        AtA += M.T @ M
    w, V = _eig_desc(AtA)
    sv = np.sqrt(np.maximum(w, 0.0))
    x = _canon(V[:, 3])
    ric = q2R(np.array([x[3], x[0], x[1], x[2]])).T
    return ric, sv, bool(calls >= window and sv[2] > 0.25), w


class InitialExRotation:
    """CalibrationExRotation: one call per processed frame with frame_count != 0"""

    def __init__(self, window):
        self.W, self.ric, self.history, self.calls = window, np.eye(3), [], 0

    def step(self, corres, delta_q_wxyz):
        Rc = solve_relative_r(corres)
        Rimu = q2R(np.asarray(delta_q_wxyz, np.float64))
        Rcg = self.ric.T @ Rimu @ self.ric
        self.history.append([R2q(Rc), R2q(Rimu), R2q(Rcg)])
        self.calls += 1
        self.ric, self.sv, ok, _ = average(self.history, self.calls, self.W)
        return ok


# ------------------------------------------------------------------------------------------------------------- generator
R_REALSENSE = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
RIC_TRUE = R_REALSENSE @ rodrigues(np.radians([3.0, -2.0, 4.0]))
TIC_TRUE = np.array([0.05, -0.02, 0.03])


class Scene:
    """rot: amplitude (rad) of yaw / pitch / roll, each a sine at about 3 rad/s (1.5 rad/s peak rate); rot = 0 is a pure translation.
    axes: factors on the three amplitudes ((1, 0, 0): yaw only, a rotation about one axis, which leaves the extrinsic rotation unobservable)"""

    def __init__(self, cfg, phase=0.0, rot=0.5, n_landmarks=1500, seed=7, ric=RIC_TRUE, tic=TIC_TRUE, axes=(1.0, 1.0, 1.0)):
        self.cfg, self.phase, self.rot, self.ric, self.tic = cfg, float(phase), float(rot), np.asarray(ric), np.asarray(tic)
        self.axes = tuple(float(a) for a in axes)
        rs = np.random.RandomState(seed)
        self.L = np.stack([rs.uniform(3.0, 9.0, n_landmarks), rs.uniform(-7, 7, n_landmarks), rs.uniform(-7, 7, n_landmarks)], 1)
        self.imu_rate, self.cam_rate, self.t0 = 200.0, 10.0, 1.0

    def pose(self, t):
        a, ph, (ky, kp, kr) = self.rot, self.phase, self.axes
        yaw, pitch, roll = a * ky * np.sin(3.0 * t + ph), a * kp * np.sin(2.6 * t + 1.3 * ph + 0.7), a * kr * np.sin(3.4 * t + 0.7 * ph + 1.9)
        cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
        Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
        Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
        p = np.array([0.4 * np.sin(1.2 * t + ph), 0.4 * np.sin(1.0 * t + 2.0 + ph), 0.2 * np.sin(1.4 * t + 0.5)])
        return p, Rz @ Ry @ Rx

    def imu(self, t_end):
        """(t, acc, gyr) at 200 Hz from 0 to t_end: finite differences of the analytic pose (vio_synth_imu's rule), no noise, no bias"""
        h, g = 1e-4, float(self.cfg.g_norm)
        ts = np.arange(0.0, t_end, 1.0 / self.imu_rate)
        acc, gyr = np.zeros((len(ts), 3)), np.zeros((len(ts), 3))
        for k, t in enumerate(ts):
            pm, Rm = self.pose(t - h)
            p0, R0 = self.pose(t)
            pp, Rp = self.pose(t + h)
            aw = (pp - 2 * p0 + pm) / (h * h) + np.array([0, 0, g])
            M = R0.T @ (Rp - Rm) / (2 * h)
            gyr[k] = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
            acc[k] = R0.T @ aw
        return ts, acc, gyr

    def frame_time(self, k):
        return self.t0 + k / self.cam_rate + 0.0025

    def frame(self, t):
        """(ids ascending, xyz_uv_vel [n][7], depth u16 [H][W]) of the frame at time t: at most max_cnt landmarks, lowest ids first"""
        c = self.cfg
        p, R = self.pose(t)
        Rwc, pwc = R @ self.ric, p + R @ self.tic
        Pc = (self.L - pwc) @ Rwc
        z = Pc[:, 2]
        ok = z > 0.5
        x, y = np.where(ok, Pc[:, 0] / np.where(ok, z, 1), 0), np.where(ok, Pc[:, 1] / np.where(ok, z, 1), 0)
        u, v = c.fx * x + c.cx, c.fy * y + c.cy
        ok &= (u >= 2) & (u < c.width - 2) & (v >= 2) & (v < c.height - 2)
        ids = np.nonzero(ok)[0][: c.max_cnt].astype(np.int32)
        obs = np.zeros((len(ids), 7))
        obs[:, 0], obs[:, 1], obs[:, 2], obs[:, 3], obs[:, 4] = x[ids], y[ids], 1.0, u[ids], v[ids]
        depth = np.zeros((c.height, c.width), np.uint16)
        depth[v[ids].astype(int), u[ids].astype(int)] = np.round(z[ids] * 1000).astype(np.uint16)
        return ids, obs, depth

    def corres(self, t_l, t_r):
        """getCorresponding(l, r) for two frames: landmarks in both feature maps, in id order"""
        i1, o1, _ = self.frame(t_l)
        i2, o2, _ = self.frame(t_r)
        common, a, b = np.intersect1d(i1, i2, return_indices=True)
        return np.hstack([o1[a, :3], o2[b, :3]])


def imu_until(ts, k0, t_frame):
    """IMU samples to push before the frame at t_frame: everything up to one sample past it (the estimator waits for t >= t_frame)"""
    k = k0
    while k < len(ts) and ts[k] <= t_frame:
        k += 1
    return min(k + 1, len(ts))


def predict_success(sc, max_frames=200):
    """the restatement on the generator's noise-free pairs (true relative body rotations as delta_q): (call count at success, ric), call k
    pairing frames k - 1 and k; (None, ric) when it does not succeed within max_frames"""
    cal = InitialExRotation(sc.cfg.window_size)
    for k in range(1, max_frames):
        tl, tr = sc.frame_time(k - 1), sc.frame_time(k)
        _, Rl = sc.pose(tl)
        _, Rr = sc.pose(tr)
        if cal.step(sc.corres(tl, tr), R2q(Rl.T @ Rr)):
            return k, cal.ric
    return None, cal.ric
