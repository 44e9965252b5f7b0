#!/usr/bin/env python
"""Replay a rosbag-free RGB-D + IMU recording through the MI355X hot path and write the reference's result CSV.

    python tools/replay.py --config <vio.yaml> --data <dir with rgb.txt depth.txt imu.txt> --out vins_result.csv [--gt gt.txt]

The recording layout is described in vins-rgbd-fast_amd/dataio.py (RgbdImuDirectory).  --gt: ``stamp x y z ...`` ground truth
(TUM format) for an ATE report.  Repeated --config / --data / --out triples replay several recordings in ONE handle, one slot each, every
slot with the calibration of its own configuration file (dataio.batch_config_from_yamls: the files must agree on every handle-wide
setting); --gt then applies to the first recording.

    --save-at FRAME --snapshot FILE   (one recording) write the sequence's snapshot after frame FRAME to FILE, the replay's own state to FILE.json
    --resume FILE                     (one recording) restore FILE and continue behind the saved frame; --out then holds the rows from there on
    --imu-rate-out FILE               (one recording) the IMU-rate poses (pubLatestOdometry: one row per IMU sample, the layout of --out)
    --keyframes-out DIR               one kf_<slot>_<stamp ns>.npz per published keyframe (pubKeyframe: pose row and rows of 8, dataio.PublicationWriter)
    --cloud-out FILE                  the last point cloud and margin cloud of every slot (pubPointCloud), one .npz"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    """(argparse namespace, [(config, data, out)]): the i-th --config, --data and --out belong together; --out may be left out (one
    recording: vins_result.csv, several: vins_result_<i>.csv)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", required=True)
    ap.add_argument("--data", action="append", required=True)
    ap.add_argument("--out", action="append", default=None)
    ap.add_argument("--gt", default=None)
    ap.add_argument("--save-at", type=int, default=None, help="frame index after which the snapshot is written (with --snapshot)")
    ap.add_argument("--snapshot", default=None, help="snapshot file to write (its sidecar FILE.json holds the frame gate's state)")
    ap.add_argument("--resume", default=None, help="snapshot file to restore before replaying the frames behind it")
    ap.add_argument("--imu-rate-out", default=None, help="file for the IMU-rate poses: one row per IMU sample, the layout of --out")
    ap.add_argument("--keyframes-out", default=None, help="directory for one .npz per published keyframe and slot")
    ap.add_argument("--cloud-out", default=None, help="file (.npz) for the last point cloud and margin cloud of every slot")
    ap.add_argument("--lenient", action="store_true", help="warn instead of failing on settings outside the built hot path")
    a = ap.parse_args(argv)
    n = len(a.config)
    if len(a.data) != n:
        ap.error("%d --config but %d --data: give one --data per --config" % (n, len(a.data)))
    if (a.save_at is None) != (a.snapshot is None):
        ap.error("--save-at and --snapshot go together")
    if n > 1 and (a.snapshot or a.resume or a.imu_rate_out):
        ap.error("--snapshot / --resume / --imu-rate-out work on one recording")
    outs = a.out if a.out is not None else (["vins_result.csv"] if n == 1 else ["vins_result_%d.csv" % i for i in range(n)])
    if len(outs) != n:
        ap.error("%d --config but %d --out: give one --out per --config, or none" % (n, len(outs)))
    return a, list(zip(a.config, a.data, outs))


def main(argv=None):
    a, triples = parse_args(argv)
    P = importlib.import_module("vins-rgbd-fast_amd")
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    pw = io.PublicationWriter(a.keyframes_out, a.cloud_out) if (a.keyframes_out or a.cloud_out) else None
    if len(triples) > 1:
        cfg, cals, extras = io.batch_config_from_yamls([t[0] for t in triples], P, strict=not a.lenient)
        for e in extras:
            for n in e["notes"]:
                print("note:", n, file=sys.stderr)
        recs = [io.RgbdImuDirectory(t[1]) for t in triples]
        b = P.VioBatch(cfg, len(triples), imu_capacity=1 << 15)
        for i, (k, e) in enumerate(zip(cals, extras)):
            b.set_calibration(i, k)
            if e["camera"] is not None:   # KANNALA_BRANDT / MEI (dataio.config_from_yaml)
                b.set_camera(i, e["camera"])
        all_rows = io.replay_many(b, recs, [t[2] for t in triples], freqs=[e["freq"] for e in extras],
                                  frontend_freqs=[e["frontend_freq"] for e in extras], publish=pw)
        for (cfg_path, data, out), rec, rows in zip(triples, recs, all_rows):
            print("%s: %d frames, %d odometry rows -> %s" % (data, len(rec), len(rows), out))
        rows = all_rows[0]
    else:
        cfg_path, data, out = triples[0]
        cfg, extra = io.config_from_yaml(cfg_path, P, strict=not a.lenient)
        for n in extra["notes"]:
            print("note:", n, file=sys.stderr)
        rec = io.RgbdImuDirectory(data)
        b = P.VioBatch(cfg, 1, imu_capacity=1 << 15)
        if extra["camera"] is not None:   # KANNALA_BRANDT / MEI (dataio.config_from_yaml)
            b.set_camera(0, extra["camera"])
        rows = io.replay(b, rec, out, freq=extra["freq"], frontend_freq=extra["frontend_freq"],
                         save_at=a.save_at, snapshot=a.snapshot, resume=a.resume,  # freq / frontend_freq: estimator_nodelet.cpp:264-286
                         imu_rate=a.imu_rate_out, publish=pw)
        print("%d frames, %d odometry rows -> %s" % (len(rec), len(rows), out))
        if a.imu_rate_out:
            print("IMU-rate poses -> %s" % a.imu_rate_out)
    if pw is not None:
        pw.close()
        print("%d keyframes -> %s, clouds -> %s" % (pw.n_keyframes, a.keyframes_out, a.cloud_out))
    if a.gt and len(rows) > 3:
        gt = np.loadtxt(a.gt, comments="#", ndmin=2)
        gp = np.array([gt[np.argmin(np.abs(gt[:, 0] - t)), 1:4] for t in rows[:, 0]])
        print("ATE rmse %.4f m over %d poses" % (io.ate_rmse(rows[:, 1:4], gp), len(rows)))


if __name__ == "__main__":
    main()
