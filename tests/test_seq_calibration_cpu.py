"""Per-sequence calibration without a GPU: the vio_calibration mirror, the config <-> calibration round trip, the configuration-file
readers for several rigs, tools/replay.py's argument pairing, and the host renderer under alternating cameras."""
import ctypes as C
import importlib
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "tests", "golden", "reference_config")


@pytest.fixture(scope="module")
def io(P):
    return importlib.import_module("vins-rgbd-fast_amd.dataio")


def test_calibration_mirror_matches_the_library(P):
    L = P.lib()
    assert L.vio_abi_version() >= 10
    assert L.vio_abi_sizeof(2) == C.sizeof(P.Calibration) == 27 * 8
    assert [f[0] for f in P.Calibration._fields_] == list(P.CALIBRATION_FIELDS)


def test_calibration_from_config_round_trip(P):
    cfg = P.default_config(fx=611.5, cy=244.25, k2=-0.3, td=-0.012, tr=0.033, acc_n=0.2, gyr_w=3e-4, g_norm=9.79)
    for i in range(3):
        cfg.tic[i] = 0.01 * (i + 1)
    k = P.Calibration()
    P.lib().vio_calibration_from_config(C.byref(cfg), C.byref(k))
    py = P.calibration_from_config(cfg)
    assert bytes(k) == bytes(py)
    for f in P.CALIBRATION_FIELDS:
        assert np.array_equal(np.array(getattr(k, f), ndmin=1), np.array(getattr(cfg, f), ndmin=1)), f
    # merging the calibration back leaves every handle-wide field of the configuration as it was
    other = P.default_config(width=848, max_cnt=120, estimate_td=1)
    merged = P.config_with_calibration(other, k)
    for name, _ in P.Config._fields_:
        src = cfg if name in P.CALIBRATION_FIELDS else other
        assert np.array_equal(np.array(getattr(merged, name), ndmin=1), np.array(getattr(src, name), ndmin=1)), name


@pytest.mark.parametrize("rel", ["realsense/vio.yaml", "realsense/vio_atlas.yaml", "realsense/vio_indoor.yaml", "realsense/vio_campus.yaml",
                                 "realsense/vio_d455.yaml", "openloris/openloris_vio.yaml"])
def test_calibration_from_yaml_reads_the_file_values(P, io, rel):
    path = os.path.join(CFG_DIR, rel)
    y = io.parse_opencv_yaml(open(path).read())
    k = io.calibration_from_yaml(path, P, strict=False)
    pp, dp = y["projection_parameters"], y["distortion_parameters"]
    for f in ("fx", "fy", "cx", "cy"):
        assert getattr(k, f) == float(pp[f]), f
    for f in ("k1", "k2", "p1", "p2"):
        assert getattr(k, f) == float(dp[f]), f
    for f in ("acc_n", "acc_w", "gyr_n", "gyr_w", "g_norm"):
        assert getattr(k, f) == float(y[f]), f
    assert k.td == float(y.get("td", 0.0))
    assert k.tr == (float(y["rolling_shutter_tr"]) if int(y.get("rolling_shutter", 0)) else 0.0)
    if int(y.get("estimate_extrinsic", 0)) == 2:
        assert list(k.ric) == list(np.eye(3).ravel()) and list(k.tic) == [0.0, 0.0, 0.0]
    else:
        assert list(k.ric) == [float(v) for v in np.asarray(y["extrinsicRotation"], np.float64).ravel()]
        assert list(k.tic) == [float(v) for v in np.asarray(y["extrinsicTranslation"], np.float64).ravel()]


def _variant(tmp_path, name, subs):
    text = open(os.path.join(CFG_DIR, "realsense", "vio.yaml")).read()
    for key, val in subs.items():
        lines = text.split("\n")
        hit = [i for i, l in enumerate(lines) if l.strip().startswith(key + ":")]
        assert hit, key
        indent = lines[hit[0]][:len(lines[hit[0]]) - len(lines[hit[0]].lstrip())]
        lines[hit[0]] = "%s%s: %s" % (indent, key, val)
        text = "\n".join(lines)
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_batch_config_accepts_files_that_differ_in_calibration(P, io, tmp_path):
    base = os.path.join(CFG_DIR, "realsense", "vio.yaml")
    other = _variant(tmp_path, "rig_b.yaml", {"fx": 640.0, "cy": 250.5, "k1": 0.0, "acc_n": 0.4, "gyr_w": 2e-4, "g_norm": 9.78, "td": -0.01,
                                              "rolling_shutter_tr": 0.02})
    cfg, cals, extras = io.batch_config_from_yamls([base, other], P)
    c0, _ = io.config_from_yaml(base, P)
    assert bytes(cfg) == bytes(c0)
    assert len(cals) == 2 and len(extras) == 2
    assert bytes(cals[0]) == bytes(io.calibration_from_yaml(base, P))
    k = cals[1]
    assert (k.fx, k.cy, k.k1, k.acc_n, k.gyr_w, k.g_norm, k.td, k.tr) == (640.0, 250.5, 0.0, 0.4, 2e-4, 9.78, -0.01, 0.02)


@pytest.mark.parametrize("pair,keys", [(("vio.yaml", "vio_atlas.yaml"), ("estimate_td",)),
                                       (("vio_indoor.yaml", "vio_campus.yaml"), ("static_init", "fix_depth", "depth_min_dist"))])
def test_batch_config_refuses_handle_wide_differences(P, io, pair, keys):
    paths = [os.path.join(CFG_DIR, "realsense", p) for p in pair]
    with pytest.raises(ValueError) as e:
        io.batch_config_from_yamls(paths, P)
    assert str(e.value).split(":")[0] in keys, str(e.value)


def test_replay_tool_pairs_its_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        replay = importlib.import_module("replay")
    finally:
        sys.path.pop(0)
    a, t = replay.parse_args(["--config", "a.yaml", "--data", "da"])
    assert t == [("a.yaml", "da", "vins_result.csv")]
    a, t = replay.parse_args(["--config", "a.yaml", "--data", "da", "--out", "oa.csv", "--config", "b.yaml", "--data", "db", "--out", "ob.csv"])
    assert t == [("a.yaml", "da", "oa.csv"), ("b.yaml", "db", "ob.csv")]
    a, t = replay.parse_args(["--config", "a.yaml", "--config", "b.yaml", "--data", "da", "--data", "db"])
    assert t == [("a.yaml", "da", "vins_result_0.csv"), ("b.yaml", "db", "vins_result_1.csv")]
    for bad in (["--config", "a.yaml", "--config", "b.yaml", "--data", "da"],
                ["--config", "a.yaml", "--data", "da", "--data", "db"],
                ["--config", "a.yaml", "--config", "b.yaml", "--data", "da", "--data", "db", "--out", "o.csv"]):
        with pytest.raises(SystemExit):
            replay.parse_args(bad)


def test_host_render_alternating_cameras_from_threads(P):
    """vio_synth_render_host keeps one ray table: threads that alternate two cameras must each render with their own camera's rays"""
    sa = P.default_synth(width=320, height=240, fx=300.0, fy=300.0, cx=160.0, cy=120.0)
    sb = P.default_synth(width=256, height=192, fx=210.0, fy=215.0, cx=131.0, cy=93.0, k1=0.1, k2=-0.2)
    jobs = [(sa if j % 2 == 0 else sb, 2 + j % 3, 1.0 + 0.05 * j) for j in range(24)]
    serial = [P.Synth(sc).render_host(seq, t) for sc, seq, t in jobs]
    out = [None] * len(jobs)

    def worker(w):
        for j in range(w, len(jobs), 6):
            sc, seq, t = jobs[j]
            out[j] = P.Synth(sc).render_host(seq, t)

    th = [threading.Thread(target=worker, args=(w,)) for w in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for j in range(len(jobs)):
        assert np.array_equal(out[j][0], serial[j][0]) and np.array_equal(out[j][1], serial[j][1]), j
