#!/usr/bin/env python
"""What one IMU-rate poll of the whole batch costs: vio_get_imu_rate_odometry / vio_get_latest_odometry_all for every
sequence of the benchmark handle against one vio_get_latest_odometry call per sequence, on the same handle in the same state.

    python tools/imu_rate_bench.py [--seqs 128] [--pending 7] [--calls 200] [--warmup 20] [--frames 14] [--out profiles/imu_rate_odometry.json]

The handle is fed --frames rendered frames (every sequence NON_LINEAR), then --pending samples per sequence are pushed (one frame
interval of a 30 Hz camera at 200 Hz), and nothing else runs: the handle is idle.  Every call ends in a stream synchronise; a figure is the
median host wall-clock over --calls calls after --warmup calls, the variants alternate call by call so that drift of the machine hits all of
them alike.  Before anything is timed the batched rows are compared with the per-sequence getter, bit for bit.  Prints one JSON line and
writes it to --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=128)
    ap.add_argument("--pending", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_rate_odometry.json"))
    a = ap.parse_args()
    P = importlib.import_module("vins-rgbd-fast_amd")
    import vio_ct
    cfg = P.canonical_config()
    S, cap = a.seqs, a.cap
    b = P.VioBatch(cfg, S)
    b.set_tracker_lag(1)   # as bench.py runs the handle
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    g, d = P.DeviceBuffer(S * cfg.width * cfg.height), P.DeviceBuffer(S * cfg.width * cfg.height * 2)
    n_imu = int(a.frames / sc.cam_rate * sc.imu_rate) + 64 + a.pending
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
    k2 = k + a.pending - 1   # one sample beyond the last frame is in the ring already
    if k2 > k:
        b.push_imu_batch(np.stack([q[0][k:k2] for q in imu]), np.stack([q[1][k:k2] for q in imu]), np.stack([q[2][k:k2] for q in imu]))
    L, h = b.L, b.h
    n_rows, rows = np.zeros(S, np.int32), np.zeros((S, cap, 11))
    one, every = np.zeros((S, 11)), np.zeros((S, 11))
    dev = P.DeviceBuffer(S * cap * 11 * 8)

    def per_sequence():
        for s in range(S):
            L.vio_get_latest_odometry(h, s, one.ctypes.data + s * 88)

    def poll():
        L.vio_get_imu_rate_odometry(h, None, cap, n_rows.ctypes.data, rows.ctypes.data, 0)

    def poll_device():
        L.vio_get_imu_rate_odometry(h, None, cap, n_rows.ctypes.data, dev.ptr, 1)

    def latest_all():
        L.vio_get_latest_odometry_all(h, every.ctypes.data, 0)

    variants = [("per_sequence_latest_odometry", per_sequence), ("imu_rate_odometry", poll), ("imu_rate_odometry_on_device", poll_device),
                ("latest_odometry_all", latest_all)]
    # same results first
    for _, fn in variants:
        fn()
    assert n_rows.min() == n_rows.max() and 0 < n_rows[0] <= cap, n_rows
    assert np.array_equal(every, one) and np.array_equal(rows[np.arange(S), n_rows - 1], one)
    assert np.array_equal(dev.download(0, (S, cap, 11), np.float64), rows)
    t = {name: [] for name, _ in variants}
    for i in range(a.warmup + a.calls):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                t[name].append(time.perf_counter() - t0)
    out = dict(seqs=S, rows_per_sequence=int(n_rows[0]), cap=cap, calls=a.calls, warmup=a.warmup)
    for name, _ in variants:
        v = np.array(t[name]) * 1e3
        out[name + "_ms"] = dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))
    base = out["per_sequence_latest_odometry_ms"]["median"]
    out["ratio_per_sequence_over_imu_rate_poll"] = base / out["imu_rate_odometry_ms"]["median"]
    out["ratio_per_sequence_over_latest_all"] = base / out["latest_odometry_all_ms"]["median"]
    dev.free()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fd:
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
