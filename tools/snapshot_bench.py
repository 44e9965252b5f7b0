#!/usr/bin/env python
"""Cost of sequence snapshots: bytes per sequence, and the host wall-clock of vio_save_seqs / vio_load_seqs for 1 sequence and
for every sequence of the benchmark handle, into pageable and into page-locked memory, beside the naive alternative the pack kernel replaces
(one hipMemcpy per layout-table entry and sequence, vio_debug_save_seq_naive).

    python tools/snapshot_bench.py [--seqs 128] [--calls 12] [--warmup 2] [--frames 0]

Every call ends in a device synchronise, the handle is idle, the figure is the median over --calls calls after --warmup calls.  --frames F
feeds F rendered frames first (the timings do not depend on the state's content; the default skips it).  Prints one JSON line."""
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


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=128)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=0)
    a = ap.parse_args()
    P = importlib.import_module("vins-rgbd-fast_amd")
    import bench
    import vio_ct
    cfg = P.canonical_config()
    S = a.seqs
    b = P.VioBatch(cfg, S)
    b.set_tracker_lag(1)   # as bench.py runs the handle
    if a.frames:
        sc = vio_ct.synth_like(cfg)
        syn = P.Synth(sc)
        g, d = P.DeviceBuffer(S * cfg.width * cfg.height), P.DeviceBuffer(S * cfg.width * cfg.height * 2)
        ti, ai, gi = syn.imu(0, int(a.frames / sc.cam_rate * sc.imu_rate) + 64)
        for s in range(S):
            tq, aq, gq = syn.imu(s, len(ti))
            b.push_imu(s, tq, aq, gq)
        for f in range(a.frames):
            syn.render_device(S, 0, f / sc.cam_rate, g.at(0), d.at(0))
            b.feed(g.at(0), d.at(0), [f / sc.cam_rate] * S, on_device=True)
        b.sync()
    per_seq = b.snapshot_bytes(0)
    out = dict(seqs=S, bytes_per_seq=per_seq, calls=a.calls, warmup=a.warmup,
               layout_state_entries=sum(1 for r in b.snapshot_layout() if r[3] >= 0))
    five = P.VioBatch(bench.config5(P), 1)
    out["bytes_per_seq_config5"] = five.snapshot_bytes(0)
    five.close()
    pinned = P.PinnedArray((per_seq * S,), np.uint8)
    for label, buf in (("pageable", np.empty(per_seq * S, np.uint8)), ("pinned", pinned.a)):
        for n in sorted({1, S}):
            seqs = np.arange(n, dtype=np.int32)
            sizes = np.full(n, per_seq, np.int64)
            offs = np.arange(n, dtype=np.int64) * per_seq          # back to back: one copy per call
            key = "%s_n%d" % (label, n)

            def save():
                assert b.L.vio_save_seqs(b.h, n, seqs.ctypes.data, buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data, None) == 0

            def load():
                assert b.L.vio_load_seqs(b.h, n, seqs.ctypes.data, buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data) == 0, b.L.vio_last_error()
            out["save_ms_" + key] = median_ms(save, a.calls, a.warmup)
            out["load_ms_" + key] = median_ms(load, a.calls, a.warmup)
            mb = per_seq * n / 1e6
            out["save_GBps_" + key] = mb / out["save_ms_" + key]
            out["load_GBps_" + key] = mb / out["load_ms_" + key]

            def naive():
                for s in seqs:
                    r = b.L.vio_debug_save_seq_naive(b.h, int(s), buf.ctypes.data + int(s) * per_seq, per_seq)
                    assert r == per_seq, r
            out["naive_save_ms_" + key] = median_ms(naive, max(3, a.calls // 3) if n > 1 else a.calls, 1)
            out["naive_save_GBps_" + key] = mb / out["naive_save_ms_" + key]
    pinned.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
