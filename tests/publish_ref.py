"""The definition of the batched publishers (vio_publish_all) in plain numpy float64: pubPointCloud's cloud and margin
cloud (visualization.cpp:328-407) and pubKeyframe's pose and 2D-3D points (visualization.cpp:454-520), from what the per-sequence getters
return and from the feature maps that were fed.

    publish(landmarks_ex rows of 12, window rows of 17, extrinsic (13), status fields, fed) -> (counts, kf_pose, cloud, margin, kf_points)

fed maps a stamp to {feature id: the observation row of 7 (x y z u v vx vy) filed under the window frame with that stamp}.  For a track
without gaps that is simply the map handed to processImage at that stamp; TrackMirror below keeps the book for the tracks where it is not
(an id that left the map and came back is filed under the next frame of its track, as upstream).

World points are written as explicit scalar products and sums in the order of Estimator::pointCloud() (include/vio_adapter.hpp): each
coordinate is ((a + b) + c) + offset.  Rs comes either from the caller (the stage tests: the same matrix the kernel is given) or from the
window's quaternion with the adapter's expansion (Estimator::refresh)."""
import numpy as np

BRANCHES = ("n_obs<2", "n_obs>=2", "start<W-2", "start>=W-2", "start>3W/4", "start<=3W/4", "solve_flag=0", "solve_flag=1", "solve_flag=2",
            "dynamic", "depth=0", "depth>0", "margin:start=0,n_obs<=2", "margin:start=0,n_obs>2", "margin:start>0", "kf:end<W-2", "kf:end>=W-2",
            "kf:dynamic", "kf:not NON_LINEAR", "kf:MARGIN_SECOND_NEW", "kf:unprocessed", "kf:valid")


def quat_to_R(q):
    """Eigen::Quaterniond::toRotationMatrix as Estimator::refresh writes it (w, x, y, z)"""
    qw, qx, qy, qz = (float(v) for v in q)
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])


def world_point(q, Rs, Ps, ric, tic):
    """(pw [3], bound [3]) of a landmark row q of 12.  bound: the sum of the absolute values of every term, per coordinate:
    (|P| + |R| (|ric| |pc| + |tic|)), the scale of the issue's rounding bound"""
    start = int(q[1])
    d = float(q[3]) if q[10] == 0 else float(q[10])
    pc = [float(q[7]) * d, float(q[8]) * d, float(q[9]) * d]
    R, P = Rs[start], Ps[start]
    pi, ai = [0.0] * 3, [0.0] * 3
    for r in range(3):
        pi[r] = float(ric[r][0]) * pc[0] + float(ric[r][1]) * pc[1] + float(ric[r][2]) * pc[2] + float(tic[r])
        ai[r] = abs(float(ric[r][0])) * abs(pc[0]) + abs(float(ric[r][1])) * abs(pc[1]) + abs(float(ric[r][2])) * abs(pc[2]) + abs(float(tic[r]))
    pw, bw = [0.0] * 3, [0.0] * 3
    for r in range(3):
        pw[r] = float(R[r][0]) * pi[0] + float(R[r][1]) * pi[1] + float(R[r][2]) * pi[2] + float(P[r])
        bw[r] = abs(float(R[r][0])) * ai[0] + abs(float(R[r][1])) * ai[1] + abs(float(R[r][2])) * ai[2] + abs(float(P[r]))
    return pw, bw


def publish(lm, window, extrinsic, status, fed, Rs=None, taken=None, with_bounds=False):
    """lm [n][12] (landmarks_ex), window [W+1][17], extrinsic [13] = tic, ric, td; status = dict or object with solver_flag,
    marginalization_flag, processed; fed as above (only read where a keyframe is published).  Rs [W+1][3][3]: the rotation matrices
    themselves where the caller has them.  taken: a set that receives the names of the BRANCHES this call went through.
    Returns (counts int32 [4], kf_pose [8] or None, cloud [n_cloud][3], margin [n_margin][3], kf_points [n_kf][8]), every list in the
    order of lm; with_bounds adds the three lists' per-coordinate bound scales."""
    lm, window, extrinsic = np.asarray(lm, np.float64).reshape(-1, 12), np.asarray(window, np.float64), np.asarray(extrinsic, np.float64)
    get = (lambda k: status[k]) if isinstance(status, dict) else (lambda k: getattr(status, k))
    W = len(window) - 1
    note = (lambda name: None) if taken is None else taken.add
    tic, ric = extrinsic[0:3], extrinsic[3:12].reshape(3, 3)
    Ps = window[:, 0:3]
    if Rs is None:
        Rs = [quat_to_R(window[i, 3:7]) for i in range(W + 1)]
    nonlinear, margin_old, processed = int(get("solver_flag")) == 1, int(get("marginalization_flag")) == 0, int(get("processed")) != 0
    kf_valid = nonlinear and margin_old and processed
    if not nonlinear:
        note("kf:not NON_LINEAR")
    if nonlinear and not margin_old:
        note("kf:MARGIN_SECOND_NEW")
    if not processed:
        note("kf:unprocessed")
    if kf_valid:
        note("kf:valid")
    cloud, margin, kf, b_cloud, b_margin, b_kf = [], [], [], [], [], []
    for q in lm:
        fid, start, n_obs, solve, dyn = int(q[0]), int(q[1]), int(q[2]), int(q[5]), q[6] != 0
        pw = None
        note("n_obs>=2" if n_obs >= 2 else "n_obs<2")
        note("start<W-2" if start < W - 2 else "start>=W-2")
        note("solve_flag=%d" % solve)
        if dyn:
            note("dynamic")
        used = (not dyn) and n_obs >= 2 and start < W - 2
        if used:
            note("start>3W/4" if start > W * 3.0 / 4.0 else "start<=3W/4")
            if not (start > W * 3.0 / 4.0) and solve == 1:
                pw, bw = world_point(q, Rs, Ps, ric, tic)
                note("depth=0" if q[10] == 0 else "depth>0")
                cloud.append(pw)
                b_cloud.append(bw)
            if start != 0:
                note("margin:start>0")
            elif n_obs > 2:
                note("margin:start=0,n_obs>2")
            elif solve == 1:
                note("margin:start=0,n_obs<=2")
                pw, bw = world_point(q, Rs, Ps, ric, tic)
                margin.append(pw)
                b_margin.append(bw)
        if kf_valid and start < W - 2 and solve == 1:
            note("kf:end>=W-2" if start + n_obs - 1 >= W - 2 else "kf:end<W-2")
            if start + n_obs - 1 >= W - 2:
                if dyn:
                    note("kf:dynamic")
                pw, bw = world_point(q, Rs, Ps, ric, tic)
                o = fed[float(window[W - 2, 16])][fid]
                kf.append(pw + [float(o[0]), float(o[1]), float(o[3]), float(o[4]), float(fid)])
                b_kf.append(bw)
    counts = np.array([len(cloud), len(margin), len(kf) if kf_valid else 0, 1 if kf_valid else 0], np.int32)
    pose = np.concatenate([[window[W - 2, 16]], window[W - 2, 0:3], window[W - 2, 3:7]]) if kf_valid else None
    out = (counts, pose, np.array(cloud).reshape(-1, 3), np.array(margin).reshape(-1, 3), np.array(kf).reshape(-1, 8))
    if with_bounds:
        return out + (np.array(b_cloud).reshape(-1, 3), np.array(b_margin).reshape(-1, 3), np.array(b_kf).reshape(-1, 3))
    return out


class TrackMirror:
    """feature_per_frame of every live landmark, rebuilt from the maps that were fed and the landmark table after each frame: an observation is
    appended to its id's track whatever frame it was made in (FeatureManager::addFeatureCheckParallax), MARGIN_OLD drops a track's first
    observation where it started in frame 0 (removeBack / removeBackShiftDepth), MARGIN_SECOND_NEW drops the one of window frame W-1
    (removeFront), and a track that left the table is gone.  The table's n_obs decides whether a slide took an observation, and must agree
    with the mirror afterwards: a track the mirror cannot explain raises."""

    def __init__(self, W, depth_min=0.0):
        self.W, self.depth_min, self.tracks = W, float(depth_min), {}

    def frame(self, ids, obs, lm, marginalization_flag, depth=None):
        """after a PROCESSED frame: the map it was given (with its depth image: an observation whose depth pixel reads 0 < d < depth_min is
        erased from the map before it is filed, feature_manager.cpp:71-80), the landmark table and the marginalisation flag it left"""
        for i, o in zip(ids, obs):
            if depth is not None:
                r, c = min(max(int(o[4]), 0), depth.shape[0] - 1), min(max(int(o[3]), 0), depth.shape[1] - 1)
                if 0 < depth[r, c] / 1000.0 < self.depth_min:
                    continue
            self.tracks.setdefault(int(i), []).append(np.array(o, np.float64))
        live = {}
        for q in np.asarray(lm).reshape(-1, 12):
            fid, start, n_obs = int(q[0]), int(q[1]), int(q[2])
            tr = self.tracks.get(fid, [])
            if len(tr) == n_obs + 1:
                tr.pop(0 if int(marginalization_flag) == 0 else self.W - 1 - start)
            if len(tr) != n_obs:
                raise AssertionError("track %d: the table holds %d observations, the fed maps explain %d" % (fid, n_obs, len(tr)))
            live[fid] = tr
        self.tracks = live

    def fed_at(self, lm, window, frame):
        """{stamp of window frame `frame`: {id: the observation filed under it}} for the landmarks whose track spans it"""
        out = {}
        for q in np.asarray(lm).reshape(-1, 12):
            fid, start, n_obs = int(q[0]), int(q[1]), int(q[2])
            if start <= frame <= start + n_obs - 1:
                out[fid] = self.tracks[fid][frame - start]
        return {float(window[frame, 16]): out}
