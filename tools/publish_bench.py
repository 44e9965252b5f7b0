#!/usr/bin/env python
"""What publishing keyframes and point clouds of the whole batch costs: one vio_publish_all call (host and HBM destination)
against what a caller had to do before it existed -- vio_get_landmarks_ex + vio_get_window + vio_get_extrinsic for every sequence, then the
filters and the world-point formula on the host -- on the same handle in the same state.

    python tools/publish_bench.py [--seqs 128] [--calls 50] [--warmup 5] [--frames 24] [--out profiles/publish_all.json]

The handle is fed --frames rendered frames (every sequence NON_LINEAR, the window full and moving) and is idle afterwards.  Every call ends in
a synchronise; a figure is the median host wall-clock over --calls calls after --warmup calls, the variants alternate call by call.  The
per-sequence loop is timed twice: the getters alone, and with the host formula (numpy, vectorised over a sequence's landmarks).  Before
anything is timed the counts of the two sides are compared.  publish_all uses cap = the landmark capacity, publish_all_tight a cap just above
the largest count (the bytes copied back grow with cap).  Prints one JSON line and writes it to --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_publish(lm, win, ex, st, W):
    """the three lists of one sequence from the getters' rows: counts and world points (the keyframe's x, y, u, v are not in any getter)"""
    tic, ric = ex[0:3], ex[3:12].reshape(3, 3)
    start, n_obs, solved, dyn = lm[:, 1].astype(int), lm[:, 2].astype(int), lm[:, 5] == 1, lm[:, 6] != 0
    used = ~dyn & (n_obs >= 2) & (start < W - 2)
    cloud = used & ~(start > W * 3.0 / 4.0) & solved
    margin = used & (start == 0) & (n_obs <= 2) & solved
    valid = st.solver_flag == 1 and st.marginalization_flag == 0 and st.processed
    kf = (start < W - 2) & (start + n_obs - 1 >= W - 2) & solved if valid else np.zeros(len(lm), bool)
    d = np.where(lm[:, 10] == 0, lm[:, 3], lm[:, 10])
    pi = (lm[:, 7:10] * d[:, None]) @ ric.T + tic
    q = win[start, 3:7]
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw), 2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz),
                  2 * (qy * qz - qx * qw), 2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(-1, 3, 3)
    pw = np.einsum("nij,nj->ni", R, pi) + win[start, 0:3]
    return pw[cloud], pw[margin], pw[kf], valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=128)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish_all.json"))
    a = ap.parse_args()
    P = importlib.import_module("vins-rgbd-fast_amd")
    import vio_ct
    cfg = P.canonical_config()
    S, W = a.seqs, cfg.window_size
    b = P.VioBatch(cfg, S)
    b.set_tracker_lag(1)   # as bench.py runs the handle
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    g, d = P.DeviceBuffer(S * cfg.width * cfg.height), P.DeviceBuffer(S * cfg.width * cfg.height * 2)
    n_imu = int(a.frames / sc.cam_rate * sc.imu_rate) + 64
    imu = [syn.imu(s, n_imu) for s in range(S)]
    k = 0
    for f in range(a.frames):
        tf = f / sc.cam_rate
        k2 = k
        while k2 < n_imu and imu[0][0][k2] <= tf + 1e-9:   # every sequence has the same stamps
            k2 += 1
        k2 = min(n_imu, k2 + 1)
        b.push_imu_batch(np.stack([q[0][k:k2] for q in imu]), np.stack([q[1][k:k2] for q in imu]), np.stack([q[2][k:k2] for q in imu]))
        k = k2
        syn.render_device(S, 0, tf, g.at(0), d.at(0))
        b.feed(g.at(0), d.at(0), [tf] * S, on_device=True)
    b.sync()
    assert all(st.solver_flag == 1 for st in b.status_all()), "not every sequence is NON_LINEAR: feed more --frames"
    L, h = b.L, b.h
    NL = b.capacity()["landmarks"]
    counts = np.zeros((S, 4), np.int32)
    pose, cloud, margin, kf = np.zeros((S, 8)), np.zeros((S, NL, 3)), np.zeros((S, NL, 3)), np.zeros((S, NL, 8))
    dev = [P.DeviceBuffer(S * 8 * 8), P.DeviceBuffer(S * NL * 3 * 8), P.DeviceBuffer(S * NL * 3 * 8), P.DeviceBuffer(S * NL * 8 * 8)]
    lm, win, ex = np.zeros((S, NL, 12)), np.zeros((S, W + 1, 17)), np.zeros((S, 13))
    n_lm = np.zeros(S, int)
    host = [None] * S

    def publish_all():
        assert L.vio_publish_all(h, NL, counts.ctypes.data, pose.ctypes.data, cloud.ctypes.data, margin.ctypes.data, kf.ctypes.data, 0) == 0

    def publish_all_on_device():
        assert L.vio_publish_all(h, NL, counts.ctypes.data, dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, 1) == 0

    def getters():
        for s in range(S):
            n_lm[s] = L.vio_get_landmarks_ex(h, s, NL, lm[s].ctypes.data)
            L.vio_get_window(h, s, win[s].ctypes.data)
            L.vio_get_extrinsic(h, s, ex[s].ctypes.data)

    def getters_and_formula():
        getters()
        sts = b.status_all()
        for s in range(S):
            host[s] = host_publish(lm[s, :n_lm[s]], win[s], ex[s], sts[s], W)

    # same results first
    publish_all()
    getters_and_formula()
    for s in range(S):
        c, m, q, valid = host[s]
        assert (len(c), len(m), len(q), int(valid)) == tuple(counts[s]), (s, counts[s])
        assert len(c) == 0 or np.abs(c - cloud[s, :len(c)]).max() < 1e-9
    first = counts.copy()
    tight = int(counts[:, :3].max()) + 8
    t_cloud, t_margin, t_kf = np.zeros((S, tight, 3)), np.zeros((S, tight, 3)), np.zeros((S, tight, 8))

    def publish_all_tight():
        assert L.vio_publish_all(h, tight, counts.ctypes.data, pose.ctypes.data, t_cloud.ctypes.data, t_margin.ctypes.data, t_kf.ctypes.data, 0) == 0

    variants = [("per_sequence_getters", getters), ("per_sequence_getters_and_host_formula", getters_and_formula), ("publish_all", publish_all),
                ("publish_all_tight", publish_all_tight), ("publish_all_on_device", publish_all_on_device)]
    t = {name: [] for name, _ in variants}
    for i in range(a.warmup + a.calls):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                t[name].append(time.perf_counter() - t0)
    assert np.array_equal(counts, first)
    out = dict(command="python tools/publish_bench.py --seqs %d --calls %d --warmup %d --frames %d" % (S, a.calls, a.warmup, a.frames), seqs=S,
               window_size=W, landmark_capacity=NL, tight_cap=tight, calls=a.calls, warmup=a.warmup, keyframes_valid=int(first[:, 3].sum()),
               mean_counts=[float(v) for v in first[:, :3].mean(0)],
               bytes_back=dict(publish_all=int(S * (16 + 64 + NL * 14 * 8)), publish_all_tight=int(S * (16 + 64 + tight * 14 * 8)),
                               publish_all_on_device=int(S * 16)))
    for name, _ in variants:
        v = np.array(t[name]) * 1e3
        out[name + "_ms"] = dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))
    base = out["per_sequence_getters_and_host_formula_ms"]["median"]
    for name in ("publish_all", "publish_all_tight", "publish_all_on_device"):
        out["ratio_per_sequence_over_" + name] = base / out[name + "_ms"]["median"]
    for x in dev + [g, d]:
        x.free()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fd:
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
