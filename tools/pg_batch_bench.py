#!/usr/bin/env python
"""Loop detection for a whole batch: one vio_pg_batch_step against the per-keyframe path for the same keyframes, in one process on the same
inputs.
    python tools/pg_batch_bench.py [--seqs 128] [--depth 200] [--warmup 3] [--steps 10] [--out profiles/pg_batch.json] [--no-serial]
S rendered 640 x 480 frames (one per sequence, every n-th FAST corner as window point) are stepped against databases `depth` entries
deep.  The databases are filled beforehand -- the batch's through vio_pg_batch_step_desc (mode 2), one Vocabulary handle per sequence
through vio_pg_db_add -- with the descriptors of a pool of rendered frames that contains the timed frames, so that the timed queries find
candidates and the match runs.  Timed with the host clock around calls that each return only after their own device
synchronisation (the device is idle at both ends of a step), median of `steps`:
  * one vio_pg_batch_step (host images in, results out);
  * S x (vio_pg_describe, vio_pg_detect_loop, vio_pg_match where there is a candidate), the old descriptors kept on the host.
Both paths see the same keyframes, so their loop decisions are compared as well.  The per-kernel share of the batched step comes from HIP
events on the batch's stream (vio_pg_batch_set_timing), taken in separate steps from the timed ones.  Needs a GPU; prints one JSON line."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bow_util  # noqa: E402
import vio_ct  # noqa: E402

POOL = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=128)
    ap.add_argument("--depth", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--max-keypoints", type=int, default=2048)
    ap.add_argument("--max-window", type=int, default=256)
    ap.add_argument("--no-serial", action="store_true", help="time the batched step only (deep databases: the serial fill takes long)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = vio_ct.pkg()
    pg = importlib.import_module("vins-rgbd-fast_amd.posegraph")
    _, L = pg._lib()
    cfg = P.canonical_config()
    syn = P.Synth(vio_ct.synth_like(cfg))
    pat = pg.load_brief_pattern(os.path.join(ROOT, "tests", "golden", "brief_pattern.npz"))
    S, MK, MW, depth = a.seqs, a.max_keypoints, a.max_window, a.depth
    H, W = cfg.height, cfg.width
    n_iter = a.warmup + a.steps
    n_prof = 5

    # the pool: POOL rendered frames, described once through the per-keyframe path
    pool = []
    for j in range(POOL):
        g, _ = syn.render_host(j % 8, 2.0 + 0.37 * j)
        _, kxy, kd, kn = pg.describe(cfg, g, np.zeros((0, 2), np.float32), pat, cap=MK)
        kxy, kd, kn = kxy[:MK], kd[:MK], kn[:MK]
        uv = np.ascontiguousarray(kxy[:: max(1, len(kxy) // 150)][:MW], np.float32)
        wd = pg.describe(cfg, g, uv, pat, cap=MK)[0]
        pool.append(dict(gray=g, kd=kd, kn=kn, uv=uv, wd=wd))
    voc = bow_util.train_vocabulary(np.concatenate([p["kd"] for p in pool]), np.concatenate([np.full(len(p["kd"]), j) for j, p in enumerate(pool)]), 10, 4, 3)
    mk_voc = lambda: pg.Vocabulary.from_arrays(voc["k"], voc["L"], 0, 0, voc["node_id"], voc["parent_id"], voc["weight"], voc["desc"], voc["word_node"],
                                               voc["word_id"])
    which = lambda s, e: (5 * s + e) % POOL                # the pool frame of entry e of sequence s; the timed steps continue the pattern

    # ---- the batch
    hb = mk_voc()
    K = depth + n_iter + n_prof + 2
    db = pg.BatchDatabase(cfg, hb, pat, S, K, MK, MW)
    for e in range(depth):
        idx = [which(s, e) for s in range(S)]
        res = db.step_desc([2] * S, [pool[i]["kd"] for i in idx], [pool[i]["kn"] for i in idx], [None] * S)
        assert all(r["status"] == 0 for r in res)
    mode = np.ones(S, np.uint8)
    out = (pg.StepOut * S)()
    bi, bd, on = np.zeros((S, MW), np.int32), np.zeros((S, MW), np.int32), np.zeros((S, MW, 2), np.float32)
    gray, uv, nw = np.zeros((S, H, W), np.uint8), np.zeros((S, MW, 2), np.float32), np.zeros(S, np.int32)

    def load(e):
        for s in range(S):
            p = pool[which(s, e)]
            gray[s], nw[s] = p["gray"], len(p["uv"])
            uv[s, :len(p["uv"])] = p["uv"]

    def batch_step():
        rc = L.vio_pg_batch_step(db.h, mode.ctypes.data, gray.ctypes.data, nw.ctypes.data, uv.ctypes.data, 0, C.addressof(out), bi.ctypes.data,
                                 bd.ctypes.data, on.ctypes.data)
        assert rc == 0, rc

    t_batch, loops_batch = [], []
    for it in range(n_iter):
        load(depth + it)
        t0 = time.perf_counter()
        batch_step()
        t_batch.append((time.perf_counter() - t0) * 1e3)
        loops_batch.append([(int(o.loop_index), int(o.n_match)) for o in out])
    db.set_timing(True)
    shares = []
    for it in range(n_prof):
        load(depth + n_iter + it)
        batch_step()
        shares.append(db.last_timing())
    db.set_timing(False)
    kern = {k: float(np.median([x[k] for x in shares])) for k in shares[0]}
    result = dict(seqs=S, depth=depth, width=W, height=H, max_keypoints=MK, max_window=MW, vocabulary="trained k=10 L=4, %d words" % len(voc["word_node"]),
                  warmup=a.warmup, steps=a.steps, keypoints_mean=float(np.mean([o.n_kp for o in out])), bow_mean=float(np.mean([o.n_bow for o in out])),
                  candidates_per_step=float(np.mean([sum(1 for l, _ in st if l != -1) for st in loops_batch[a.warmup:]])),
                  batch_step_ms=float(np.median(t_batch[a.warmup:])), batch_step_ms_all=[round(x, 3) for x in t_batch[a.warmup:]],
                  kernel_ms=kern, kernel_share={k: (v / kern["total"] if kern["total"] > 0 else 0.0) for k, v in kern.items() if k != "total"})
    db.close(); hb.close()

    # ---- the per-keyframe path on the same keyframes
    if not a.no_serial:
        vocs = [mk_voc() for _ in range(S)]
        for s in range(S):
            for e in range(depth):
                vocs[s].add(pool[which(s, e)]["kd"])
        wd, kxy, kd, kn = np.zeros((MW, 4), np.uint64), np.zeros((MK, 2), np.float32), np.zeros((MK, 4), np.uint64), np.zeros((MK, 2), np.float32)
        sbi, sbd = np.zeros(MW, np.int32), np.zeros(MW, np.int32)
        loop, ids, scs, nret = C.c_int32(-1), np.zeros(4, np.int32), np.zeros(4), C.c_int32(0)
        t_serial, loops_serial = [], []
        for it in range(n_iter):
            load(depth + it)
            dec = []
            t0 = time.perf_counter()
            for s in range(S):
                n = int(nw[s])
                m = L.vio_pg_describe(C.byref(cfg), gray[s].ctypes.data, n, uv[s].ctypes.data, pat.ctypes.data, 20, wd.ctypes.data, MK, kxy.ctypes.data,
                                      kd.ctypes.data, kn.ctypes.data)
                assert m >= 0
                m = min(m, MK)
                rc = L.vio_pg_detect_loop(vocs[s].h, kd.ctypes.data, m, depth + it, C.addressof(loop), ids.ctypes.data, scs.ctypes.data, C.addressof(nret))
                assert rc == 0
                nm = 0
                if loop.value != -1:
                    old = pool[which(s, loop.value)]["kd"]     # the host keeps every keyframe's descriptors for this
                    rc = L.vio_pg_match(wd.ctypes.data, n, old.ctypes.data, len(old), sbi.ctypes.data, sbd.ctypes.data)
                    assert rc == 0
                    nm = int((sbi[:n] >= 0).sum())
                dec.append((int(loop.value), nm))
            t_serial.append((time.perf_counter() - t0) * 1e3)
            loops_serial.append(dec)
        for v in vocs:
            v.close()
        result.update(serial_step_ms=float(np.median(t_serial[a.warmup:])), serial_step_ms_all=[round(x, 3) for x in t_serial[a.warmup:]],
                      same_decisions=bool(loops_serial == loops_batch))
        result["ratio"] = result["serial_step_ms"] / result["batch_step_ms"]
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not a.no_serial and not (result["same_decisions"] and result["batch_step_ms"] < result["serial_step_ms"]):
        sys.exit(1)                                        # the batched step must compute the same and be faster


if __name__ == "__main__":
    main()
