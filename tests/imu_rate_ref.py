"""Plain-numpy definition of the IMU-rate odometry rows (Estimator::predict, estimator.cpp:1862-1880, applied from the newest window
state through every IMU sample newer than it: what pubLatestOdometry publishes, one row per sample).  The replay of
test_gpu_parity2.py::test_latest_odometry_with_the_reference_replay_quirk, for both modes and with every intermediate row kept."""
import numpy as np


def q2R(q):
    """Eigen's toRotationMatrix formula, no normalisation (w, x, y, z)"""
    a, b, c, d = q
    return np.array([[1 - 2 * (c * c + d * d), 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), 1 - 2 * (b * b + d * d), 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), 1 - 2 * (b * b + c * c)]])


def R2q(m):
    """Eigen's Quaternion(Matrix3) (w, x, y, z)"""
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
    v = np.zeros(3)
    v[i] = 0.5 * t
    t = 0.5 / t
    w = (m[k, j] - m[j, k]) * t
    v[j] = (m[j, i] + m[i, j]) * t
    v[k] = (m[k, i] + m[i, k]) * t
    return np.array([w, v[0], v[1], v[2]])


def imu_rate_rows(w_row, td, g, ti, ai, gi, n_buffered, quirk):
    """w_row: the newest window row [P(3) Q(wxyz) V(3) Ba(3) Bg(3) stamp]; td: the estimated time offset; g: the gravity vector (3);
    ti, ai, gi: EVERY sample pushed so far; n_buffered: how many of them had been pushed when the last frame was processed; quirk:
    reference_quirks bit 0 (VIO_QUIRK_LATEST_FRONT).
    Returns (rows [n][11], state [11]): one row t, P, Q(wxyz), V per sample newer than stamp + td, and the window state itself in the same
    layout (what comes back when no sample is applied)."""
    w_row, ti, ai, gi, g = (np.asarray(x, np.float64) for x in (w_row, ti, ai, gi, g))
    t0 = w_row[16] + td
    R, P, V, Ba, Bg = q2R(w_row[3:7]), w_row[0:3].copy(), w_row[7:10].copy(), w_row[10:13], w_row[13:16]
    state = np.r_[t0, P, R2q(R), V]
    # the queue's front = the first sample processImage did not pop = the first one with t >= Headers[W] + td (getIMUInterval keeps it);
    # it is also the last sample processIMU consumed for the newest frame: acc_0 / gyr_0
    at_or_after = np.nonzero(ti >= t0)[0]
    rows = []
    if len(at_or_after):
        front = int(at_or_after[0])
        a0, g0 = ai[front].copy(), gi[front].copy()
        lt = t0
        for i in np.nonzero(ti > t0)[0]:
            dt = ti[i] - lt
            lt = ti[i]
            # quirk: samples that were buffered when the last frame was processed are replayed by updateLatestStates with the FRONT sample's
            # values (:1779-1786), later ones go through inputIMU -> predict with their own (:1758-1764), and predict() never advances
            # acc_0 / gyr_0.  Default: every sample with its own values, which become acc_0 / gyr_0 of the next step.
            src = front if (quirk and i < n_buffered) else i
            un_acc_0 = R @ (a0 - Ba) - g
            th = (0.5 * (g0 + gi[src]) - Bg) * dt
            R = R @ q2R(np.array([1.0, th[0] / 2, th[1] / 2, th[2] / 2]))   # Utility::deltaQ, not normalised (utility.h:11-24)
            un_acc = 0.5 * (un_acc_0 + R @ (ai[src] - Ba) - g)
            P = P + dt * V + 0.5 * dt * dt * un_acc
            V = V + dt * un_acc
            if not quirk:
                a0, g0 = ai[src], gi[src]
            rows.append(np.r_[lt, P, R2q(R), V])
    return np.array(rows).reshape(-1, 11), state
