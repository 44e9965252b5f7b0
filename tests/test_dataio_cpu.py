"""CPU tests of the ROS-free configuration / dataset I/O: YAML keys of readParameters, the result CSV
format of pubOdometry, recording round trip."""
import glob
import importlib
import os

import numpy as np
import pytest

import vio_ct

REF_CONFIG = os.path.join(vio_ct.ROOT, "tests", "golden", "reference_config")

YAML = """%YAML:1.0
# written for this test: the key set of parameters.cpp:81-243 with values of our own
imu: 1
static_init: 1
imu_topic: "/imu0"     # strings may carry a # inside quotes: "/a#b"
image_topic: "/cam/color"
output_path: "/tmp/out"
depth_min_dist: 0.25
depth_max_dist: 7.5
fix_depth: 0
num_grid_rows: 7
num_grid_cols: 8
model_type: PINHOLE
image_width: 848
image_height: 480
distortion_parameters:
   k1: 0.01
   k2: -0.02
   p1: 0.003
   p2: -0.004
projection_parameters:
   fx: 430.5
   fy: 431.5
   cx: 424.25
   cy: 240.75
estimate_extrinsic: 1
extrinsicRotation: !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [ 0.0, 0.0, 1.0,
           -1.0, 0.0, 0.0,
           0.0, -1.0, 0.0 ]
extrinsicTranslation: !!opencv-matrix
   rows: 3
   cols: 1
   dt: d
   data: [ 0.1, 0.02, -0.03 ]
max_cnt: 150
min_dist: 15
freq: 10
F_threshold: 1.5
show_track: 0
equalize: 0
fisheye: 0
max_solver_time: 0.04
max_num_iterations: 6
keyframe_parallax: 8.0
acc_n: 0.2
gyr_n: 0.02
acc_w: 0.002
gyr_w: 0.0002
g_norm: 9.81
estimate_td: 1
td: -0.005
rolling_shutter: 1
rolling_shutter_tr: 0.033
"""


@pytest.fixture(scope="module")
def io():
    return importlib.import_module("vins-rgbd-fast_amd.dataio")


def test_yaml_keys_map_to_vio_config(P, io):
    cfg, extra = io.config_from_yaml(YAML, P)
    assert (cfg.width, cfg.height, cfg.max_cnt, cfg.min_dist, cfg.grid_rows, cfg.grid_cols) == (848, 480, 150, 15, 7, 8)
    assert (cfg.fix_depth, cfg.estimate_extrinsic, cfg.estimate_td, cfg.max_iterations) == (0, 1, 1, 6)
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (430.5, 431.5, 424.25, 240.75)
    assert (cfg.k1, cfg.k2, cfg.p1, cfg.p2) == (0.01, -0.02, 0.003, -0.004)
    assert (cfg.depth_min, cfg.depth_max, cfg.f_threshold, cfg.min_parallax_px) == (0.25, 7.5, 1.5, 8.0)
    assert (cfg.acc_n, cfg.gyr_n, cfg.acc_w, cfg.gyr_w, cfg.g_norm) == (0.2, 0.02, 0.002, 0.0002, 9.81)
    assert list(cfg.ric) == [0, 0, 1, -1, 0, 0, 0, -1, 0] and list(cfg.tic) == [0.1, 0.02, -0.03]
    assert (cfg.td, cfg.tr) == (-0.005, 0.033)
    assert extra["freq"] == 10 and extra["output_path"] == "/tmp/out" and extra["notes"] == []
    y = io.parse_opencv_yaml(YAML)
    assert y["imu_topic"] == "/imu0" and y["extrinsicRotation"].shape == (3, 3) and y["extrinsicTranslation"].shape == (3, 1)


def test_static_init_zero_selects_the_dynamic_initialisation(P, io):
    """static_init: 0 (config/realsense/vio_campus.yaml:10, openloris_vio.yaml:10) -> vio_config.dynamic_init = 1 (parameters.cpp:167)"""
    txt = "\n".join(l for l in YAML.splitlines() if not l.startswith("static_init:")) + "\nstatic_init: 0\n"
    cfg, extra = io.config_from_yaml(txt, P)
    assert cfg.dynamic_init == 1 and extra["notes"] == []
    assert io.config_from_yaml(YAML, P)[0].dynamic_init == 0


def test_imu_zero_selects_vo_mode(P, io):
    """imu: 0 (config/tum_rgbd/tum_fr3.yaml:9) -> use_imu 0, LK maxLevel 3 (feature_tracker.cpp:307-311)"""
    txt = "\n".join(l for l in YAML.splitlines() if not l.startswith("imu:")) + "\nimu: 0\n"
    cfg, extra = io.config_from_yaml(txt, P)
    assert (cfg.use_imu, cfg.lk_max_level, cfg.estimate_td) == (0, 3, 0) and extra["notes"] == []
    assert io.config_from_yaml(YAML, P)[0].use_imu == 1


def test_equalize_selects_clahe(P, io):
    """equalize: 1 (parameters.cpp:110) -> vio_config.equalize, the CLAHE branch of readImage (feature_tracker.cpp:269-275)"""
    txt = "\n".join(l for l in YAML.splitlines() if not l.startswith("equalize:")) + "\nequalize: 1\n"
    cfg, extra = io.config_from_yaml(txt, P)
    assert cfg.equalize == 1 and extra["notes"] == []
    assert io.config_from_yaml(YAML, P)[0].equalize == 0


def test_fisheye_names_the_mask_file(P, io):
    """fisheye: 1 (parameters.cpp:111-114) -> the caller decodes config/fisheye_mask.jpg and hands it to VioBatch.set_fisheye_mask"""
    txt = "\n".join(l for l in YAML.splitlines() if not l.startswith("fisheye:")) + "\nfisheye: 1\n"
    assert io.config_from_yaml(txt, P)[1]["fisheye_mask"] == "config/fisheye_mask.jpg"
    assert io.config_from_yaml(YAML, P)[1]["fisheye_mask"] is None


@pytest.mark.parametrize("line,what", [("model_type: KANNALA_BRANDT", "camera model"), ("estimate_extrinsic: 2", "extrinsic")])
def test_out_of_scope_settings_fail_loudly(P, io, line, what):
    key = line.split(":")[0]
    txt = "\n".join(l for l in YAML.splitlines() if not l.startswith(key + ":")) + "\n" + line + "\n"
    with pytest.raises(ValueError):
        io.config_from_yaml(txt, P)
    cfg, extra = io.config_from_yaml(txt, P, strict=False)
    assert len(extra["notes"]) == 1


def test_reference_config_files_parse(P, io):
    """every VIO configuration the reference ships parses (its config/ files, copied as data under tests/golden/reference_config)"""
    files = sorted(glob.glob(os.path.join(REF_CONFIG, "**", "*.yaml"), recursive=True))
    files = [f for f in files if "vio" in os.path.basename(f) or "rgbd" in os.path.basename(f).lower()]
    assert len(files) == 8, files
    n_ok = 0
    for f in files:
        y = io.parse_opencv_yaml(open(f).read())
        if "max_cnt" not in y:
            continue
        cfg, extra = io.config_from_yaml(f, P, strict=False)
        assert cfg.width >= 320 and cfg.height >= 240 and cfg.max_cnt > 0 and cfg.fx > 100
        R = np.array(cfg.ric[:]).reshape(3, 3)
        assert abs(np.linalg.det(R) - 1) < 1e-3
        n_ok += 1
    assert n_ok >= 3
    cfg, _ = io.config_from_yaml(os.path.join(REF_CONFIG, "realsense", "vio.yaml"), P, strict=False)
    d = P.default_config()
    assert (cfg.width, cfg.height, cfg.grid_rows, cfg.grid_cols) == (640, 480, 5, 6)
    for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "g_norm", "gyr_n", "acc_w", "gyr_w"):
        assert getattr(cfg, k) == getattr(d, k), k  # vio_config_default mirrors this file (except max_cnt / min_dist / acc_n: DESIGN.md)
    assert list(cfg.ric) == list(d.ric) and list(cfg.tic) == list(d.tic)


def test_csv_row_format(io, tmp_path):
    row = io.format_odometry_row(1403636579.763555527, [1.234567, -0.000004, 10.0], [0.707106781, 0.0, -0.707106781, 0.000001], [0.1, -2.5, 3.333335])
    assert row == "1403636579763555584,1.23457,-0.00000,10.00000,0.70711,0.00000,-0.70711,0.00000,0.10000,-2.50000,3.33333,\n"
    p = tmp_path / "r.csv"
    w = io.OdometryCsvWriter(str(p), append=False)
    w.write_rows(np.arange(22, dtype=np.float64).reshape(2, 11) * 0.5)
    w.close()
    back = io.read_odometry_csv(str(p))
    assert back.shape == (2, 11) and np.allclose(back, np.arange(22).reshape(2, 11) * 0.5, atol=1e-5)


def test_gray_conversion_is_opencv_fixed_point(io):
    rgb = np.zeros((2, 3, 3), np.uint8)
    rgb[0, 0] = (255, 255, 255); rgb[0, 1] = (255, 0, 0); rgb[0, 2] = (0, 255, 0); rgb[1, 0] = (0, 0, 255); rgb[1, 1] = (12, 200, 99)
    g = io.rgb_to_gray(rgb)
    assert g[0, 0] == 255 and g[0, 1] == 76 and g[0, 2] == 150 and g[1, 0] == 29
    assert g[1, 1] == (12 * 4899 + 200 * 9617 + 99 * 1868 + 8192) >> 14
    assert np.array_equal(io.rgb_to_gray(g), g)


def test_recording_round_trip(P, io, tmp_path):
    cfg = P.default_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    stamps = [0.0, 0.1, 0.2]
    fr = [syn.render_host(2, t) for t in stamps]
    ti, ai, gi = syn.imu(2, 60)
    io.write_recording(str(tmp_path), stamps, [f[0] for f in fr], [f[1] for f in fr], ti, ai, gi)
    rec = io.RgbdImuDirectory(str(tmp_path))
    assert len(rec) == 3 and np.array_equal(rec.imu_t, ti) and np.array_equal(rec.imu_acc, ai) and np.array_equal(rec.imu_gyr, gi)
    for k in range(3):
        t, g, d = rec.frame(k)
        assert t == stamps[k] and np.array_equal(g, fr[k][0]) and np.array_equal(d, fr[k][1]) and d.dtype == np.uint16


def test_ate_alignment(io):
    rng = np.random.default_rng(0)
    gt = rng.normal(size=(50, 3))
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    est = (R @ gt.T).T + [3.0, -2.0, 0.5]
    assert io.ate_rmse(est, gt) < 1e-12
    assert abs(io.ate_rmse(est + [0, 0, 0.1] * (np.arange(50) % 2)[:, None], gt) - 0.05) < 1e-3


def _stamp_streams():
    rng = np.random.default_rng(4)
    out = []
    for rate in (10.0, 20.0, 30.0, 60.0):
        t = 5.0 + np.arange(400) / rate
        out.append(t)
        out.append(t + rng.normal(0, 0.1 / rate, t.shape))          # jittered stamps
    gap = np.r_[np.arange(60) / 30.0, 5.0 + np.arange(60) / 30.0, 4.0 + np.arange(30) / 30.0]   # a hole, then a jump back in time
    out.append(gap)
    return out


@pytest.mark.parametrize("freq,frontend_freq", [(10, 20), (10, 30), (30, 30), (0, 30), (20, 15)])
def test_frame_gate_python_equals_oracle_restatement(freq, frontend_freq):
    """dataio.FrameGate (product host side) against the oracle's restatement of estimator_nodelet.cpp:234-286 on regular, jittered and
    discontinuous stamp streams, with empty-map events injected at the same frames."""
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    import vio_ct
    for t in _stamp_streams():
        a, b = io.FrameGate(freq, frontend_freq), vio_ct.OracleGate(freq, frontend_freq)
        da, db = [], []
        for k, x in enumerate(t):
            da.append(a.step(x)); db.append(b.step(x))
            if k % 37 == 36 and da[-1] == 2:
                a.empty_map(x); b.empty_map(x)
        assert da == db
        if freq == 10 and frontend_freq >= 20:
            assert 2 in da and 3 in da


def test_frame_gate_cpp_header_equals_oracle_restatement(tmp_path):
    """vio_hip::FrameGate of include/vio_adapter.hpp (what a nodelet links) on the same streams."""
    import subprocess
    import vio_ct
    src = tmp_path / "gate.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "vio_adapter.hpp"\nint main(int c, char **v) { vio_hip::FrameGate g(atoi(v[1]), atoi(v[2])); '
                   'double t; int k = 0; while (scanf("%lf", &t) == 1) { int d = (int)g.step(t); printf("%d\\n", d); if (k % 37 == 36 && d == 2) g.emptyMap(t); k++; } return 0; }\n')
    exe = str(tmp_path / "gate")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(root, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for freq, ff in [(10, 20), (10, 30), (0, 30)]:
        for t in _stamp_streams():
            out = subprocess.run([exe, str(freq), str(ff)], input="\n".join("%.17g" % x for x in t), capture_output=True, text=True)
            dc = [int(x) for x in out.stdout.split()]
            b = vio_ct.OracleGate(freq, ff)
            db = []
            for k, x in enumerate(t):
                db.append(b.step(x))
                if k % 37 == 36 and db[-1] == 2:
                    b.empty_map(x)
            assert dc == db


def _jittered_pairs(seed):
    """colour stamps at 30 Hz; depth stamps = colour + jitter, with some depth / colour frames missing and two stamp clusters far apart"""
    rng = np.random.default_rng(seed)
    tc = np.arange(120) / 30.0 + 10.0
    td = tc + rng.choice([0.0, 0.001, -0.002, 0.0029, -0.0031, 0.004, -0.006, 0.012], size=len(tc))
    keep_c = rng.random(len(tc)) > 0.08
    keep_d = rng.random(len(td)) > 0.08
    return tc[keep_c], np.sort(td[keep_d])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_color_depth_pairing_python_equals_oracle_restatement(seed):
    """dataio.ColorDepthSync / pair_color_depth (product host side) against the oracle's restatement of estimator_nodelet.cpp:200-232
    on jittered and gappy stamp lists: the same pairs, the same number of thrown colour / depth frames, both drop branches exercised,
    and every pair within the 3 ms tolerance."""
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    import vio_ct
    tc, td = _jittered_pairs(seed)
    got = io.pair_color_depth(tc, td)
    ref, thrown_c, thrown_d = vio_ct.oracle_pair_color_depth(tc, td)
    assert got == ref and len(got) > 40
    assert thrown_c > 0 and thrown_d > 0
    assert all(abs(tc[i] - td[j]) <= 0.003 + 1e-12 for i, j in got)
    # online use: messages arrive interleaved in stamp order, pairs come out as soon as both queues hold a message
    sync = io.ColorDepthSync()
    ev = sorted([(t, 0, i) for i, t in enumerate(tc)] + [(t, 1, j) for j, t in enumerate(td)])
    online = []
    for t, kind, idx in ev:
        (sync.push_color if kind == 0 else sync.push_depth)(t, idx)
        while True:
            p = sync.pop()
            if p is None:
                break
            online.append((p[0][1], p[1][1]))
    assert online == ref and (sync.thrown_color, sync.thrown_depth) <= (thrown_c, thrown_d)


def test_color_depth_pairing_cpp_header_equals_oracle_restatement(tmp_path):
    """vio_hip::ColorDepthSync of include/vio_adapter.hpp (what a nodelet links) on the same stamp lists."""
    import subprocess
    import vio_ct
    src = tmp_path / "sync.cpp"
    src.write_text('#include <cstdio>\n#include "vio_adapter.hpp"\nint main() { vio_hip::ColorDepthSync<int> s; int nc, nd; double t; if (scanf("%d %d", &nc, &nd) != 2) return 1;\n'
                   'for (int i = 0; i < nc; i++) { if (scanf("%lf", &t) != 1) return 1; s.pushColor(t, i); }\n'
                   'for (int j = 0; j < nd; j++) { if (scanf("%lf", &t) != 1) return 1; s.pushDepth(t, j); }\n'
                   'int c, d; double tc; while (s.pop(c, d, tc)) printf("%d %d\\n", c, d); printf("-1 %d\\n-1 %d\\n", s.thrown_color, s.thrown_depth); return 0; }\n')
    exe = str(tmp_path / "sync")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in (0, 1, 2):
        tc, td = _jittered_pairs(seed)
        out = subprocess.run([exe], input="%d %d\n" % (len(tc), len(td)) + "\n".join("%.17g" % x for x in np.r_[tc, td]), capture_output=True, text=True)
        rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.strip().splitlines()]
        ref, thrown_c, thrown_d = vio_ct.oracle_pair_color_depth(tc, td)
        assert rows[:-2] == ref and rows[-2] == (-1, thrown_c) and rows[-1] == (-1, thrown_d)


def test_recording_with_jittered_depth_stamps_pairs_like_the_nodelet(tmp_path):
    """RgbdImuDirectory on a recording whose depth stamps are offset from the colour stamps: frames beyond +-3 ms are dropped by the
    nodelet's rule (estimator_nodelet.cpp:206-226), the others keep the COLOUR stamp; pairing="nearest" keeps them all."""
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    n = 12
    stamps = 5.0 + np.arange(n) / 10.0
    off = np.array([0, 0.001, -0.002, 0.005, 0, 0.0029, -0.004, 0, 0.0031, 0, -0.001, 0.002])
    g = [np.full((8, 8), k, np.uint8) for k in range(n)]
    d = [np.full((8, 8), 1000 + k, np.uint16) for k in range(n)]
    imu_t = 5.0 + np.arange(300) / 200.0
    io.write_recording(str(tmp_path / "r"), stamps, g, d, imu_t, np.zeros((300, 3)), np.zeros((300, 3)), depth_stamps=stamps + off)
    rec = io.RgbdImuDirectory(str(tmp_path / "r"))
    expect = [k for k in range(n) if abs(off[k]) <= 0.003]
    assert len(rec) == len(expect) == 9
    for q, k in enumerate(expect):
        t, gray, depth = rec.frame(q)
        assert abs(t - stamps[k]) < 1e-9 and gray[0, 0] == k and depth[0, 0] == 1000 + k
    assert (rec.thrown_color, rec.thrown_depth) == (3, 3)
    assert len(io.RgbdImuDirectory(str(tmp_path / "r"), pairing="nearest")) == n
    assert len(io.RgbdImuDirectory(str(tmp_path / "r"), 0.05, pairing="nearest")) == n      # max_dt is the second positional argument, as before
    # a recording the +-3 ms rule mostly rejects says so instead of silently replaying a handful of frames
    io.write_recording(str(tmp_path / "u"), stamps, g, d, imu_t, np.zeros((300, 3)), np.zeros((300, 3)), depth_stamps=stamps + 0.01)
    with pytest.warns(RuntimeWarning, match="not hardware-synchronised"):
        assert len(io.RgbdImuDirectory(str(tmp_path / "u"))) == 0


def test_pose_graph_save_and_load_round_trip(tmp_path):
    """PoseGraph::savePoseGraph / loadPoseGraph (pose_graph.cpp:849-1043): the text format of pose_graph.txt, <i>_briefdes.dat (256 characters
    per descriptor, bit 255 first, as boost::dynamic_bitset prints) and <i>_keypoints.txt; loaded keyframes are sequence 0 with the loop-closed
    pose as their VIO pose and go into the vocabulary database in order.  No GPU: the keyframes are built from saved fields, the vocabulary is a
    stand-in that records what it is given."""
    import importlib
    pg = importlib.import_module("vins-rgbd-fast_amd.posegraph")

    class Voc:
        def __init__(self):
            self.added = []

        def add(self, d):
            self.added.append(np.array(d, copy=True))
    rng = np.random.default_rng(4)

    def rot(a, b, c):
        ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
        return np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])
    g = pg.PoseGraph(Voc(), np.eye(3), np.zeros(3))
    for i in range(5):
        nk = int(rng.integers(0, 40)) if i != 2 else 0
        kf = pg.KeyFrame.from_saved(10.0 + 0.1 * i, i, rng.normal(size=3), rot(*rng.normal(size=3)), rng.normal(size=3), rot(*(3 * rng.normal(size=3))),
                                    -1 if i < 4 else 1, rng.normal(size=8) if i == 4 else np.zeros(8), rng.uniform(0, 640, (nk, 2)), rng.normal(size=(nk, 2)),
                                    rng.integers(0, 2 ** 63, (nk, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nk, 4), dtype=np.uint64))
        kf.vio_T_w_i = kf.T_w_i + 0.01 * i                       # a live graph keeps both poses
        g.keyframelist.append(kf)
    g.savePoseGraph(str(tmp_path))
    line = open(tmp_path / "pose_graph.txt").readline()
    assert line.startswith(" 0 10.000000 ") and len(line.split()) == 26
    first = open(tmp_path / "0_briefdes.dat").readline().strip() if len(g.keyframelist[0].keypoints) else "0" * 256
    assert len(first) == 256 and set(first) <= {"0", "1"}
    if len(g.keyframelist[0].keypoints):
        assert first[-1] == str(int(g.keyframelist[0].brief_descriptors[0][0]) & 1)            # bit 0 is printed last
    h = pg.PoseGraph(Voc(), np.eye(3), np.zeros(3))
    assert h.loadPoseGraph(str(tmp_path)) == 5 and h.global_index == 5 and h.earliest_loop_index == 1
    for a, b in zip(g.keyframelist, h.keyframelist):
        assert b.sequence == 0 and b.index == a.index and abs(b.time_stamp - a.time_stamp) < 1e-6
        assert np.abs(b.T_w_i - a.T_w_i).max() < 1e-6 and np.abs(b.R_w_i - a.R_w_i).max() < 3e-6   # six decimals of t and q
        assert np.array_equal(b.vio_T_w_i, b.T_w_i)                                                 # the load constructor's rule
        assert b.has_loop == a.has_loop and b.loop_index == a.loop_index and np.abs(b.loop_info - a.loop_info).max() < 1e-6
        assert np.array_equal(b.brief_descriptors, a.brief_descriptors) and b.keypoints.shape == a.keypoints.shape
        assert len(a.keypoints) == 0 or (np.abs(b.keypoints - a.keypoints).max() < 1e-4 and np.abs(b.keypoints_norm - a.keypoints_norm).max() < 1e-5)
    assert len(h.voc.added) == 5 and all(np.array_equal(x, kf.brief_descriptors) for x, kf in zip(h.voc.added, g.keyframelist))
    assert h.loadPoseGraph(str(tmp_path / "nothing_here")) == 0
