"""Sequence snapshots, the part that needs no GPU: ABI version and exports, the struct mirrors, vio_snapshot_info's refusals (also under the host
compiler's address / undefined-behaviour sanitizers on a CPU build of csrc/snapshot_host.cpp), and the shape key."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_and_exports(P):
    L = P.lib()
    assert L.vio_abi_version() >= 12
    for name in ("vio_snapshot_bytes", "vio_save_seqs", "vio_load_seqs", "vio_snapshot_info", "vio_shape_key", "vio_debug_save_seq_naive",
                 "vio_debug_snapshot_staging_bytes", "vio_debug_snapshot_layout"):
        assert hasattr(L, name), name
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vio_abi.h")).read(), flags=re.S)
    assert "vio_snapshot_header" in src and "vio_snapshot_shape" in src


def test_struct_mirrors_have_the_library_s_size(P):
    L = P.lib()
    assert L.vio_abi_sizeof(4) == C.sizeof(P.SnapshotHeader) == 208
    assert L.vio_abi_sizeof(5) == C.sizeof(P.SnapshotShape) == 144
    assert C.sizeof(P.SnapshotHeader) % 16 == 0          # the device part behind it starts on a 16-byte boundary
    assert L.vio_abi_sizeof(0) == C.sizeof(P.Config) and L.vio_abi_sizeof(6) == -1


def _header(P, cfg=None, device_bytes=64, host_bytes=48):
    hd = P.SnapshotHeader()
    hd.magic, hd.format_version, hd.abi_version = P.SNAPSHOT_MAGIC, P.SNAPSHOT_FORMAT, 12
    hd.device_bytes, hd.host_bytes = device_bytes, host_bytes
    hd.total_bytes = C.sizeof(hd) + device_bytes + host_bytes
    hd.shape = P.shape_key(cfg or P.canonical_config())
    return hd


def _blob(hd, pad=None):
    n = int(hd.total_bytes) if pad is None else pad
    out = np.zeros(max(n, C.sizeof(hd)), np.uint8)
    out[:C.sizeof(hd)] = np.frombuffer(bytes(hd), np.uint8)
    return out[:n] if pad is not None else out


def _refusal_cases(P):
    good = _header(P)
    ok = _blob(good)
    cases = [("empty", b""), ("bytes", ok[:10].tobytes()), ("bytes", ok[:C.sizeof(good) - 1].tobytes())]
    bad = ok.copy(); bad[0] ^= 0xFF
    cases.append(("magic", bad))
    fut = _header(P); fut.format_version = P.SNAPSHOT_FORMAT + 1
    cases.append(("format_version", _blob(fut)))
    zero = _header(P); zero.format_version = 0
    cases.append(("format_version", _blob(zero)))
    cases.append(("total_bytes", ok[:-1]))                                   # truncated by one byte
    cases.append(("total_bytes", ok[:C.sizeof(good)]))                        # the header alone
    lie = _header(P); lie.total_bytes += 16
    cases.append(("total_bytes", _blob(lie)))
    neg = _header(P); neg.device_bytes = -16; neg.total_bytes = C.sizeof(neg) - 16 + 48
    cases.append(("total_bytes", _blob(neg, pad=400)))
    huge = _header(P); huge.device_bytes = 1 << 62; huge.host_bytes = 1 << 62; huge.total_bytes = C.c_int64(C.sizeof(huge) + (1 << 62) + (1 << 62)).value
    cases.append(("total_bytes", _blob(huge, pad=400)))
    odd = _header(P, device_bytes=72)
    cases.append(("total_bytes", _blob(odd)))
    lag = _header(P); lag.tracker_lag = 3
    cases.append(("tracker_lag", _blob(lag)))
    return ok, cases


def test_snapshot_info_accepts_and_refuses(P):
    ok, cases = _refusal_cases(P)
    hd = P.snapshot_info(ok)
    assert hd.total_bytes == ok.size and hd.device_bytes == 64 and hd.host_bytes == 48 and hd.shape.width == 640
    assert P.snapshot_info(np.concatenate([ok, np.zeros(100, np.uint8)])).total_bytes == ok.size     # a longer buffer is fine
    assert P.snapshot_info(ok.tobytes()).magic == P.SNAPSHOT_MAGIC
    L = P.lib()
    assert L.vio_snapshot_info(None, 100, None) == P.VIO_EINVAL and L.vio_snapshot_info(ok.ctypes.data, -5, None) == P.VIO_EINVAL
    assert L.vio_snapshot_info(ok.ctypes.data, ok.size, None) == 0            # `out` is optional
    for field, blob in cases:
        with pytest.raises(P.VioError) as ei:
            P.snapshot_info(blob)
        assert field in str(ei.value), (field, str(ei.value))


SAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vio_abi.h"
/* argv[1]: a file of records "<int64 bytes><bytes...>"; every record is handed to vio_snapshot_info in a heap block of EXACTLY its size, so a
 * read past `bytes` is a heap-buffer-overflow under the address sanitizer.  Prints one result code per record. */
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    long long n;
    if (argc < 2 || !f) return 2;
    while (fread(&n, sizeof(n), 1, f) == 1) {
        unsigned char *p = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
        vio_snapshot_header hd;
        if (n > 0 && fread(p, 1, (size_t)n, f) != (size_t)n) return 3;
        printf("%d\n", vio_snapshot_info(n > 0 ? p : NULL, n, &hd));
        free(p);
    }
    {
        vio_config c;
        vio_snapshot_shape k;
        memset(&c, 0, sizeof(c));
        c.width = 640; c.max_cnt = 150;
        int rc = vio_shape_key(&c, 10, &k), cap = k.imu_capacity;
        printf("%d %d %d\n", rc, cap, vio_shape_key(NULL, 0, &k));
    }
    return 0;
}
"""


def test_snapshot_info_never_reads_past_bytes_under_sanitizers(P, tmp_path):
    """csrc/snapshot_host.cpp is plain C++: built here with the host compiler, -fsanitize=address,undefined, and run on every case of the
    refusal test in heap blocks of exactly `bytes` bytes."""
    ok, cases = _refusal_cases(P)
    blobs = [ok] + [np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b for _, b in cases]
    with open(tmp_path / "cases.bin", "wb") as fd:
        for b in blobs:
            fd.write(np.int64(b.size).tobytes()); fd.write(b.tobytes())
    (tmp_path / "main.c").write_text(SAN_MAIN)
    exe = str(tmp_path / "san")
    csrc = os.path.join(ROOT, "vins-rgbd-fast_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = "-I" + os.path.join(ROOT, "include")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-DVIO_SNAPSHOT_STANDALONE", inc, "-c", os.path.join(csrc, "snapshot_host.cpp"),
                        "-o", str(tmp_path / "host.o")] + san, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", str(tmp_path / "main.c"), "-o", str(tmp_path / "main.o")] + san,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", str(tmp_path / "main.o"), str(tmp_path / "host.o"), "-o", exe] + san, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "0" and lines[1:len(blobs)] == [str(P.VIO_EINVAL)] * len(cases), lines
    assert lines[len(blobs)] == "0 256 %d" % P.VIO_EINVAL


KEY_FIELDS = dict(width=848, height=400, max_cnt=120, min_dist=25, grid_rows=4, grid_cols=5, window_size=12, max_landmarks=800, fix_depth=0,
                  estimate_extrinsic=1, estimate_td=1, max_iterations=6, ransac_max_iters=500, lk_max_level=3, dynamic_init=1, use_imu=0,
                  reference_quirks=1, marg_exact=2, equalize=1, focal_length=400.0, f_threshold=2.0, depth_min=0.5, depth_max=7.0,
                  min_parallax_px=12.0, init_depth=4.0)


def test_shape_key_follows_the_handle_wide_fields_only(P):
    base = P.default_config()
    k0 = bytes(P.shape_key(base, 8192))
    assert bytes(P.shape_key(base, 8192)) == k0 and len(k0) == 144
    seen = {k0}
    for field, value in KEY_FIELDS.items():
        assert getattr(base, field) != value, field
        k = P.shape_key(P.default_config(**{field: value}), 8192)
        assert bytes(k) != k0 and getattr(k, field) == value, field
        seen.add(bytes(k))
    assert len(seen) == len(KEY_FIELDS) + 1                      # every field moves the key its own way
    # the IMU ring: part of the key as vio_create rounds it
    assert bytes(P.shape_key(base, 4096)) != k0 and P.shape_key(base, 10).imu_capacity == 256 == P.shape_key(base, 256).imu_capacity
    assert P.shape_key(base).hist_cap == 2048 and P.shape_key(base).pyramid_levels == 3 and list(P.shape_key(base).reserved) == [0, 0]
    # no calibration field, and nothing about a camera model or the batch size, is in the key
    for field in P.CALIBRATION_FIELDS:
        c = P.default_config()
        if field in ("ric", "tic"):
            getattr(c, field)[0] += 0.125
        else:
            setattr(c, field, getattr(c, field) + 0.125)
        assert bytes(P.shape_key(c, 8192)) == k0, field
    names = {n for n, _ in P.SnapshotShape._fields_}
    assert not names & set(P.CALIBRATION_FIELDS) and not names & {"n_seq", "S", "model"}
    # every vio_config field is either in the key or a calibration field: a new handle-wide field cannot be forgotten
    cfg_fields = {n for n, _ in P.Config._fields_}
    assert cfg_fields - set(P.CALIBRATION_FIELDS) == names - {"imu_capacity", "hist_cap", "pyramid_levels", "reserved"}
    assert set(KEY_FIELDS) == cfg_fields - set(P.CALIBRATION_FIELDS)


def test_replay_tool_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay as R
    a, triples = R.parse_args(["--config", "c.yaml", "--data", "d", "--save-at", "40", "--snapshot", "s.bin"])
    assert (a.save_at, a.snapshot, a.resume) == (40, "s.bin", None) and triples == [("c.yaml", "d", "vins_result.csv")]
    a, _ = R.parse_args(["--config", "c.yaml", "--data", "d", "--resume", "s.bin"])
    assert a.resume == "s.bin" and a.save_at is None
    for bad in (["--save-at", "3"], ["--snapshot", "x"]):
        with pytest.raises(SystemExit):
            R.parse_args(["--config", "c.yaml", "--data", "d"] + bad)
    with pytest.raises(SystemExit):
        R.parse_args(["--config", "a", "--data", "b", "--config", "c", "--data", "d", "--resume", "x"])


def test_frame_gate_state_round_trips_through_json():
    import importlib
    import json
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    g = io.FrameGate(10, 30)
    stamps = np.arange(50) / 30.0
    for t in stamps[:23]:
        g.step(t)
    h = io.FrameGate(10, 30)
    h.set_state(json.loads(json.dumps(g.state())))
    assert h.state() == g.state() and set(g.state()) == {"first_image_flag", "first_image_time", "last_image_time", "pub_count", "input_count"}
    assert [g.step(t) for t in stamps[23:]] == [h.step(t) for t in stamps[23:]]
