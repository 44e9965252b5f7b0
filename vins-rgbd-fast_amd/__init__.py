"""MI355X-native VIO hot path — Python host side (ctypes over the C ABI in include/vio_abi.h).

The package directory name contains hyphens, so import it with
``importlib.import_module("vins-rgbd-fast_amd")`` (``__graft_entry__.load_package()`` does that).

Nothing here computes on the CPU: every call ends in ``libvio_hip.so`` and fails with ``VioError`` when the
extension is missing or no GPU is present.  PyTorch is optional and only used as a source of device pointers.

Mirrors of the reference interface (same names / argument meaning):
  FeatureTracker.readImage / updateID      vins_estimator/src/feature_tracker/feature_tracker.h:36-47
  Estimator.inputIMU / processImage / ...   vins_estimator/src/estimator/estimator.h:29-60
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libvio_hip.so")

VIO_OK, VIO_NEED_IMU, VIO_REBOOTED = 0, 1, 2
VIO_EINVAL, VIO_EDEVICE, VIO_ECAPACITY = -1, -2, -3


class VioError(RuntimeError):
    pass


class Config(C.Structure):
    """vio_config (include/vio_abi.h); same field order as oracle ovio::Config."""
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "max_cnt", "min_dist", "grid_rows", "grid_cols", "window_size", "max_landmarks", "fix_depth",
        "estimate_extrinsic", "estimate_td", "max_iterations", "ransac_max_iters", "lk_max_level", "dynamic_init", "use_imu", "reference_quirks",
        "marg_exact", "equalize")] + \
        [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal_length", "f_threshold", "depth_min",
                                   "depth_max", "acc_n", "acc_w", "gyr_n", "gyr_w", "g_norm")] + \
        [("ric", C.c_double * 9), ("tic", C.c_double * 3)] + \
        [(n, C.c_double) for n in ("td", "tr", "min_parallax_px", "init_depth")]


CALIBRATION_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "ric", "tic", "td", "tr", "acc_n", "acc_w", "gyr_n", "gyr_w", "g_norm")


class Calibration(C.Structure):
    """vio_calibration (include/vio_abi.h): the per-sequence sensor calibration of a VioBatch slot."""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")] + \
        [("ric", C.c_double * 9), ("tic", C.c_double * 3)] + \
        [(n, C.c_double) for n in ("td", "tr", "acc_n", "acc_w", "gyr_n", "gyr_w", "g_norm")]


def _copy_fields(dst, src, names=CALIBRATION_FIELDS):
    for n in names:
        v = getattr(src, n)
        if n in ("ric", "tic"):
            arr = getattr(dst, n)
            for i in range(len(arr)):
                arr[i] = float(v[i])
        else:
            setattr(dst, n, float(v))
    return dst


def calibration_from_config(cfg):
    """vio_calibration_from_config: the calibration fields of a Config."""
    return _copy_fields(Calibration(), cfg)


def config_with_calibration(cfg, cal):
    """A copy of cfg with cal's fields merged in (every other field, handle-wide, unchanged)."""
    c = Config()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(Config))
    return _copy_fields(c, cal)


CAMERA_PINHOLE, CAMERA_KANNALA_BRANDT, CAMERA_MEI = 0, 1, 2
CAMERA_PARAMS = {CAMERA_PINHOLE: ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"),
                 CAMERA_KANNALA_BRANDT: ("k2", "k3", "k4", "k5", "mu", "mv", "u0", "v0"),
                 CAMERA_MEI: ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")}


class Camera(C.Structure):
    """vio_camera (include/vio_abi.h): a slot's camera model; p holds CAMERA_PARAMS[model] in order, zeros after them."""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 12)]

    def params(self):
        """{name: value} of the model's parameters"""
        return {n: float(self.p[i]) for i, n in enumerate(CAMERA_PARAMS[int(self.model)])}

    def __eq__(self, other):
        return isinstance(other, Camera) and int(self.model) == int(other.model) and list(self.p) == list(other.p)

    def __repr__(self):
        return "Camera(%d, %s)" % (int(self.model), self.params())


def _camera(model, values):
    c = Camera()
    c.model = model
    for i, v in enumerate(values):
        c.p[i] = float(v)
    return c


def camera_pinhole(cal):
    """The PINHOLE Camera of a Calibration's (or Config's) fx fy cx cy k1 k2 p1 p2"""
    return _camera(CAMERA_PINHOLE, [getattr(cal, n) for n in CAMERA_PARAMS[CAMERA_PINHOLE]])


def camera_kannala_brandt(k2, k3, k4, k5, mu, mv, u0, v0):
    """KANNALA_BRANDT (camodocal EquidistantCamera) projection_parameters"""
    return _camera(CAMERA_KANNALA_BRANDT, (k2, k3, k4, k5, mu, mv, u0, v0))


def camera_mei(xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0):
    """MEI (camodocal CataCamera): mirror_parameters xi, distortion_parameters k1 k2 p1 p2, projection_parameters gamma1 gamma2 u0 v0"""
    return _camera(CAMERA_MEI, (xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0))


def _stage_camera(fn, cam, uv, R=None):
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    n = len(uv)
    ray, un, uvo = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros((n, 2))
    Rm = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    rc = fn(C.byref(cam), n, uv.ctypes.data, None if Rm is None else Rm.ctypes.data, ray.ctypes.data, un.ctypes.data, uvo.ctypes.data)
    if rc != 0:
        raise VioError("camera stage failed (%d): %s" % (rc, lib().vio_last_error().decode()))
    return ray, un, uvo


def stage_camera(cam, uv, R=None):
    """vio_stage_camera (device): (ray [n][3] = liftProjective, un [n][2] = (x / z, y / z), uv_out [n][2] = spaceToPlane(R * ray))"""
    return _stage_camera(lib().vio_stage_camera, cam, uv, R)


def stage_host_camera(cam, uv, R=None):
    """vio_stage_host_camera: the same on the CPU (no GPU needed)"""
    return _stage_camera(lib().vio_stage_host_camera, cam, uv, R)


SNAPSHOT_MAGIC, SNAPSHOT_FORMAT = 0x0050414E534F4956, 1


class SnapshotShape(C.Structure):
    """vio_snapshot_shape (include/vio_abi.h): the shape key of a handle; two handles exchange snapshots exactly when their keys are equal."""
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "max_cnt", "min_dist", "grid_rows", "grid_cols", "window_size", "max_landmarks", "fix_depth",
        "estimate_extrinsic", "estimate_td", "max_iterations", "ransac_max_iters", "lk_max_level", "dynamic_init", "use_imu",
        "reference_quirks", "marg_exact", "equalize", "imu_capacity", "hist_cap", "pyramid_levels")] + [("reserved", C.c_int32 * 2)] + \
        [(n, C.c_double) for n in ("focal_length", "f_threshold", "depth_min", "depth_max", "min_parallax_px", "init_depth")]


class SnapshotHeader(C.Structure):
    """vio_snapshot_header (include/vio_abi.h): what every snapshot blob starts with."""
    _fields_ = [("magic", C.c_uint64), ("format_version", C.c_uint32), ("abi_version", C.c_uint32), ("total_bytes", C.c_int64),
                ("device_bytes", C.c_int64), ("host_bytes", C.c_int64), ("frames_processed", C.c_int64), ("last_stamp", C.c_double),
                ("tracker_lag", C.c_int32), ("solver_flag", C.c_int32), ("shape", SnapshotShape)]


def shape_key(cfg, imu_capacity=8192):
    """vio_shape_key: the SnapshotShape of a handle created with (cfg, imu_capacity).  Host only: needs no GPU."""
    k = SnapshotShape()
    if lib().vio_shape_key(C.byref(cfg), int(imu_capacity), C.byref(k)) != 0:
        raise VioError("vio_shape_key failed: %s" % lib().vio_last_error().decode())
    return k


def snapshot_info(blob):
    """vio_snapshot_info: validates a snapshot blob (bytes or a uint8 array) and returns its SnapshotHeader.  Host only: needs no GPU."""
    a = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, np.uint8).reshape(-1)
    hd = SnapshotHeader()
    if lib().vio_snapshot_info(a.ctypes.data if a.size else None, a.size, C.byref(hd)) != 0:
        raise VioError("vio_snapshot_info failed: %s" % lib().vio_last_error().decode())
    return hd


class SynthConfig(C.Structure):
    """vio_synth_config (include/vio_synth.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)] + \
        [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")] + \
        [("ric", C.c_double * 9), ("tic", C.c_double * 3)] + \
        [(n, C.c_double) for n in ("g_norm", "imu_rate", "cam_rate", "t_static", "acc_noise", "gyr_noise", "acc_bias_walk",
                                   "gyr_bias_walk")] + [("seed", C.c_uint64)]


class Status(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "code", "solver_flag", "frame_count", "marginalization_flag", "n_landmarks", "last_track_num", "n_tracks", "processed",
        "iterations", "successful_steps", "n_in_problem", "n_residuals", "n_var_landmarks", "has_prior", "reboot_count",
        "frames_processed")] + [(n, C.c_double) for n in ("initial_cost", "final_cost", "td")] + \
        [(n, C.c_int32) for n in ("overflow_flags", "overflow_frames", "iterations_total", "solves_total")]


FRAME_SKIP, FRAME_TRACK, FRAME_PUBLISH = 0, 1, 2


PUBLISH_BLOCK = 256   # VIO_PUBLISH_BLOCK: landmarks per step of the publishers' list walk
_PUBLISH_INT = ("lm_order", "lm_id", "lm_start", "lm_nobs", "lm_solve_flag", "lm_dyn")
_PUBLISH_F64 = ("lm_depth", "lm_obs", "Ps", "Rs", "Headers", "ric", "tic")


class PublishTables(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PUBLISH_INT + _PUBLISH_F64]


class MargStageIn(C.Structure):
    """vio_marg_stage_in (include/vio_abi.h)"""
    _fields_ = [("t", PublishTables), ("lm_est_flag", C.c_void_p)] + \
        [(n, C.c_int32) for n in ("n_lm", "ring_base", "marginalization_flag", "has_prior")] + \
        [(n, C.c_void_p) for n in ("Vs", "Bas", "Bgs", "g")] + [("td", C.c_double)] + \
        [(n, C.c_void_p) for n in ("prior_present", "prior_H", "prior_r", "prior_x0", "pre_idx", "imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_acc0",
                                   "imu_gyr0", "imu_ba", "imu_bg")]


class MargStageOut(C.Structure):
    """vio_marg_stage_out (include/vio_abi.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("prior_H", "prior_r", "prior_x0", "prior_present", "prior_c0", "has_prior", "dbg5", "margA", "margB", "margV",
                                          "b_r", "hbm_valid")]


class SolveStageOut(C.Structure):
    """vio_solve_stage_out (include/vio_abi.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("scal_i", "scal_d", "X", "Xc", "feat", "cfeat", "var_slots", "H", "g", "sp", "Hpl", "Hll", "gl", "sl", "Sc",
                                          "dgp", "dgl", "gnp", "gnl", "stp", "stl")]


SOLVE_STOP = dict(none=0, asm_a=1, schur=2, serial=3, ls=4)   # VIO_SOLVE_STOP_*
_SOLVE_SCAL_I = ("stage", "iter", "iters_done", "F", "Fa", "nres", "ex_active", "td_active", "vext", "constrained", "fused")
_SOLVE_SCAL_D = ("cost", "ccost", "radius", "mu", "alpha", "dogleg_norm", "model_change")
PS_STAGES = ("idle", "eval_x0", "asm", "schur", "step", "eval_c", "done")   # SolveSt::stage


def stage_publish(tables, W, n_lm, ring_base, flags, cap, fill=None, lists=(True, True, True)):
    """vio_stage_publish: the publishers' device routine on the tables of one synthetic sequence.  tables: dict of lm_order, lm_id, lm_start,
    lm_nobs, lm_solve_flag, lm_dyn ([NL] integers), lm_depth [NL], lm_obs [NL, W+1, 9], Ps [W+1, 3], Rs [W+1, 3, 3], Headers [W+1], ric [3, 3],
    tic [3]; flags = (solver_flag, marginalization_flag, processed).  Returns (counts [4], kf_pose [8], cloud [cap, 3], margin [cap, 3],
    kf_points [cap, 8]) with every output pre-filled with `fill` (NaN by default; counts with -1), so what the kernel left alone still holds
    it; lists[i] = False passes NULL for that list (it is counted only, and returned as None)."""
    W, n_lm, ring_base, cap = int(W), int(n_lm), int(ring_base), int(cap)
    if cap < 0:
        raise ValueError("cap must be >= 0")
    if not 2 <= W <= 20:
        raise ValueError("W must be in 2 .. 20")
    NL = len(np.asarray(tables["lm_order"]).reshape(-1))
    if NL < 1:
        raise ValueError("the tables must hold at least one slot")
    shapes = dict(lm_depth=NL, lm_obs=NL * (W + 1) * 9, Ps=3 * (W + 1), Rs=9 * (W + 1), Headers=W + 1, ric=9, tic=3)
    keep, t = [], PublishTables()
    for name in _PUBLISH_INT + _PUBLISH_F64:
        a = np.ascontiguousarray(tables[name], np.int32 if name in _PUBLISH_INT else np.float64).reshape(-1)
        if a.size != shapes.get(name, NL):
            raise ValueError("%s holds %d values, expected %d" % (name, a.size, shapes.get(name, NL)))
        keep.append(a)
        setattr(t, name, a.ctypes.data)
    f = np.ascontiguousarray(flags, np.int32).reshape(-1)
    if f.size != 3:
        raise ValueError("flags = (solver_flag, marginalization_flag, processed)")
    fill = np.nan if fill is None else float(fill)
    counts, pose = np.full(4, -1, np.int32), np.full(8, fill)
    out = [np.full((cap, w), fill) if on else None for w, on in zip((3, 3, 8), lists)]
    L = lib()
    rc = L.vio_stage_publish(NL, W, n_lm, ring_base, C.byref(t), f.ctypes.data, cap, counts.ctypes.data, pose.ctypes.data, *[_ptr(o) for o in out])
    if rc != 0:
        raise VioError("vio_stage_publish failed (%d): %s" % (rc, L.vio_last_error().decode()))
    return counts, pose, out[0], out[1], out[2]


def build(verbose=False):
    """Compile libvio_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-j8", "-C", os.path.join(_HERE, "csrc")], capture_output=True, text=True)
    if r.returncode != 0:
        raise VioError("hipcc build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return _LIB_PATH


_lib = None


def lib():
    """Load libvio_hip.so (no CPU fallback: raises if the extension is missing)."""
    global _lib
    if _lib is None:
        path = _LIB_PATH
        if os.environ.get("VIO_HIP_LIB") == "timers":
            # the profiling tools' build with the in-kernel phase timers compiled in (csrc/Makefile target `timers`); never the default
            path = os.path.join(_HERE, "libvio_hip_timers.so")
            if not os.path.exists(path):
                r = subprocess.run(["make", "-j8", "-C", os.path.join(_HERE, "csrc"), "timers"], capture_output=True, text=True)
                if r.returncode != 0:
                    raise VioError("hipcc build (timers) failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
        if not os.path.exists(path):
            raise VioError("libvio_hip.so is not built: run __graft_entry__.build() (the product path has no CPU fallback)")
        L = C.CDLL(path)
        L.vio_create.restype = C.c_void_p
        L.vio_create.argtypes = [C.POINTER(Config), C.c_int, C.c_int]
        L.vio_create_on_device.restype = C.c_void_p
        L.vio_create_on_device.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int]
        L.vio_get_device.argtypes = [C.c_void_p]
        L.vio_host_buffers_done.argtypes = [C.c_void_p, C.c_int]
        L.vio_destroy.argtypes = [C.c_void_p]
        L.vio_last_error.restype = C.c_char_p
        L.vio_reset.argtypes = [C.c_void_p]
        L.vio_push_imu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_track.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.vio_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.vio_sync.argtypes = [C.c_void_p]
        L.vio_reset_seq.argtypes = [C.c_void_p, C.c_int]
        L.vio_reset_tracker_seq.argtypes = [C.c_void_p, C.c_int]
        L.vio_set_relo_frame.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_get_relo.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_push_imu_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_feed_modes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_track_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_predict_motion.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
        L.vio_process_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        L.vio_process_obs_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_get_packaged.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.vio_get_capacity.argtypes = [C.c_void_p, C.c_void_p]
        L.vio_get_landmarks_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vio_get_odometry_history.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vio_get_stream.restype = C.c_void_p
        L.vio_get_stream.argtypes = [C.c_void_p]
        L.vio_get_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(Status)]
        L.vio_get_window.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_get_odometry.argtypes = [C.c_void_p, C.c_void_p]
        L.vio_get_extrinsic.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_calibration_from_config.argtypes = [C.POINTER(Config), C.POINTER(Calibration)]
        L.vio_set_calibration.argtypes = [C.c_void_p, C.c_int, C.POINTER(Calibration)]
        L.vio_get_calibration.argtypes = [C.c_void_p, C.c_int, C.POINTER(Calibration)]
        L.vio_set_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera)]
        L.vio_get_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera)]
        L.vio_stage_camera.argtypes = [C.POINTER(Camera), C.c_int] + [C.c_void_p] * 5
        L.vio_stage_host_camera.argtypes = [C.POINTER(Camera), C.c_int] + [C.c_void_p] * 5
        L.vio_synth_render_host_camera.argtypes = [C.POINTER(SynthConfig), C.POINTER(Camera), C.c_uint64, C.c_double, C.c_void_p, C.c_void_p]
        L.vio_synth_render_device_camera.argtypes = [C.POINTER(SynthConfig), C.POINTER(Camera), C.c_int, C.c_uint64, C.c_double, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        L.vio_shape_key.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(SnapshotShape)]
        L.vio_snapshot_info.argtypes = [C.c_void_p, C.c_int64, C.POINTER(SnapshotHeader)]
        L.vio_snapshot_bytes.restype = C.c_int64
        L.vio_snapshot_bytes.argtypes = [C.c_void_p, C.c_int]
        L.vio_save_seqs.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.vio_load_seqs.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.vio_debug_save_seq_naive.restype = C.c_int64
        L.vio_debug_save_seq_naive.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.vio_debug_snapshot_staging_bytes.restype = C.c_int64
        L.vio_debug_snapshot_staging_bytes.argtypes = [C.c_void_p]
        L.vio_debug_snapshot_layout.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if L.vio_abi_sizeof(4) != C.sizeof(SnapshotHeader) or L.vio_abi_sizeof(5) != C.sizeof(SnapshotShape):
            raise VioError("vio_snapshot_header mirror does not match the library (%d != %d bytes)" % (C.sizeof(SnapshotHeader), L.vio_abi_sizeof(4)))
        if L.vio_abi_sizeof(2) != C.sizeof(Calibration):
            raise VioError("vio_calibration mirror does not match the library (%d != %d bytes)" % (C.sizeof(Calibration), L.vio_abi_sizeof(2)))
        L.vio_get_latest_odometry.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_get_latest_odometry_all.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.vio_get_imu_rate_odometry.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_publish_all.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        L.vio_stage_publish.argtypes = [C.c_int] * 4 + [C.POINTER(PublishTables), C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.vio_set_tracker_lag.argtypes = [C.c_void_p, C.c_int]
        L.vio_set_fisheye_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.vio_get_status_all.argtypes = [C.c_void_p, C.c_void_p]
        L.vio_get_tracks.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.vio_get_landmarks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vio_get_prior.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.vio_get_timings.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_profile_begin.argtypes = [C.c_void_p, C.c_int]
        L.vio_profile_end.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vio_synth_pose.argtypes = [C.POINTER(SynthConfig), C.c_uint64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_synth_imu.argtypes = [C.POINTER(SynthConfig), C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_synth_render_host.argtypes = [C.POINTER(SynthConfig), C.c_uint64, C.c_double, C.c_void_p, C.c_void_p]
        L.vio_synth_render_device.argtypes = [C.POINTER(SynthConfig), C.c_int, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_stage_pyr_down.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vio_stage_clahe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vio_stage_fast_roi.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
        L.vio_lk_effective_level.argtypes = [C.c_int, C.c_int, C.c_int]
        L.vio_stage_lk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_stage_ransac.argtypes = [C.POINTER(Config), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_stage_relative_r.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.vio_get_ex_calibration.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.vio_stage_imu_factor.argtypes = [C.POINTER(Config), C.c_int] + [C.c_void_p] * 14
        L.vio_stage_projection.argtypes = [C.POINTER(Config)] + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                                                  C.c_int, C.c_void_p, C.c_void_p]
        L.vio_device_alloc.restype = C.c_void_p
        L.vio_device_alloc.argtypes = [C.c_size_t]
        L.vio_device_free.argtypes = [C.c_void_p]
        L.vio_device_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vio_device_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vio_stage_projection_residual.argtypes = L.vio_stage_projection.argtypes
        L.vio_stage_pnp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_stage_pnp_trace.argtypes = [C.c_int] + [C.c_void_p] * 5
        L.vio_stage_host_pnp_trace.argtypes = [C.c_int] + [C.c_void_p] * 5
        L.vio_stage_rodrigues.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.vio_stage_host_rodrigues.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.vio_stage_relative_r_detail.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vio_stage_imu_block.argtypes = [C.POINTER(Config), C.c_int] + [C.c_void_p] * 12
        L.vio_stage_chol.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.vio_stage_preint.argtypes = [C.POINTER(Config), C.c_int, C.c_int] + [C.c_void_p] * 10
        L.vio_stage_preint_ring.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_double, C.c_double] + [C.c_void_p] * 8
        L.vio_stage_imu_raw.argtypes = [C.POINTER(Config)] + [C.c_void_p] * 10
        L.vio_stage_projection_pair.argtypes = [C.POINTER(Config)] + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vio_stage_pose_ops.argtypes = [C.c_int] + [C.c_void_p] * 5
        _lib = L
    return _lib


def default_config(**kw):
    c = Config()
    lib().vio_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def canonical_config(**kw):
    """BASELINE config 2/3: 640x480, 150 features, 5x6 grid, W = 10; landmarks are optimisation variables
    (fix_depth 0, depth range as in config/realsense/vio_campus.yaml which is the upstream 150-feature setting)."""
    d = dict(fix_depth=0, depth_max=10.0)
    d.update(kw)
    return default_config(**d)


def default_synth(**kw):
    c = SynthConfig()
    lib().vio_synth_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):  # torch tensor (device or host)
        return a.data_ptr()
    return a


class PinnedArray:
    """numpy array over page-locked host memory (vio_host_alloc): hand `.a` to feed / track / process with on_device=False"""

    def __init__(self, shape, dtype):
        self.L = lib()
        self.L.vio_host_alloc.restype = C.c_void_p
        self.L.vio_host_alloc.argtypes = [C.c_size_t]
        self.L.vio_host_free.argtypes = [C.c_void_p]
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self.L.vio_host_alloc(n)
        if not self.ptr:
            raise VioError("vio_host_alloc(%d) failed" % n)
        self.a = np.frombuffer((C.c_uint8 * n).from_address(self.ptr), dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.a = None
            self.L.vio_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """A plain HBM allocation (vio_device_alloc) for the on_device = True paths when the caller has no HIP binding of its own
    (bench.py uses torch tensors instead).  `ptr` is the device address; slices are addressed with `at(byte_offset)`."""

    def __init__(self, nbytes):
        self.L = lib()
        self.nbytes = int(nbytes)
        self.ptr = self.L.vio_device_alloc(self.nbytes)
        if not self.ptr:
            raise VioError("vio_device_alloc(%d) failed: %s" % (self.nbytes, self.L.vio_last_error().decode()))

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def download(self, byte_offset, shape, dtype):
        out = np.empty(shape, dtype)
        if self.L.vio_device_download(out.ctypes.data, self.ptr + int(byte_offset), out.nbytes) != 0:
            raise VioError("vio_device_download failed")
        return out

    def upload(self, byte_offset, arr):
        arr = np.ascontiguousarray(arr)
        if self.L.vio_device_upload(self.ptr + int(byte_offset), arr.ctypes.data, arr.nbytes) != 0:
            raise VioError("vio_device_upload failed")

    def free(self):
        if self.ptr:
            self.L.vio_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Synth:
    """Synthetic RGB-D + IMU workload."""

    def __init__(self, cfg=None):
        self.cfg = cfg or default_synth()
        self.L = lib()

    def pose(self, seq, t):
        p, R, v = np.zeros(3), np.zeros(9), np.zeros(3)
        self.L.vio_synth_pose(C.byref(self.cfg), seq, t, p.ctypes.data, R.ctypes.data, v.ctypes.data)
        return p, R.reshape(3, 3), v

    def imu(self, seq, n):
        t, a, g = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        self.L.vio_synth_imu(C.byref(self.cfg), seq, n, t.ctypes.data, a.ctypes.data, g.ctypes.data)
        return t, a, g

    def render_host(self, seq, t, camera=None):
        """camera: a Camera to render through (vio_synth_render_host_camera) instead of the configuration's pinhole"""
        g = np.zeros((self.cfg.height, self.cfg.width), np.uint8)
        d = np.zeros((self.cfg.height, self.cfg.width), np.uint16)
        if camera is None:
            self.L.vio_synth_render_host(C.byref(self.cfg), seq, t, g.ctypes.data, d.ctypes.data)
        else:
            self.L.vio_synth_render_host_camera(C.byref(self.cfg), C.byref(camera), seq, t, g.ctypes.data, d.ctypes.data)
        return g, d

    def render_device(self, n_seq, seq0, t, d_gray, d_depth, stream=None, camera=None):
        if camera is None:
            rc = self.L.vio_synth_render_device(C.byref(self.cfg), n_seq, seq0, t, _ptr(d_gray), _ptr(d_depth), stream)
        else:
            rc = self.L.vio_synth_render_device_camera(C.byref(self.cfg), C.byref(camera), n_seq, seq0, t, _ptr(d_gray), _ptr(d_depth), stream)
        if rc != 0:
            raise VioError("vio_synth_render_device failed (%d)" % rc)


class VioBatch:
    """A batch of S independent sequences resident in HBM (vio_batch)."""

    def __init__(self, cfg=None, n_seq=1, imu_capacity=8192, device=None):
        """device: HIP device index the handle lives on (None = the calling thread's current device); the handle keeps it and every call
        binds to it (vio_create_on_device), so handles on different GPUs can be driven from one thread or from one thread each."""
        self.L = lib()
        self.cfg = cfg or default_config()
        self.S = n_seq
        self.W = self.cfg.window_size
        self.h = self.L.vio_create_on_device(C.byref(self.cfg), n_seq, imu_capacity, -1 if device is None else int(device))
        if not self.h:
            raise VioError("vio_create failed: %s" % self.L.vio_last_error().decode())
        self.h = C.c_void_p(self.h)
        # the calibration each slot was given, before the library re-orthonormalises ric: config_of() hands it on, so that a handle or the
        # oracle built from that configuration applies the same re-orthonormalisation to the same input
        self._cal_in = [calibration_from_config(self.cfg) for _ in range(n_seq)]

    def set_calibration(self, seq, cal):
        """vio_set_calibration: slot seq gets its own sensor calibration (a Calibration) and restarts like a fresh handle"""
        if not isinstance(cal, Calibration):
            raise TypeError("set_calibration takes a Calibration")
        self._chk(self.L.vio_set_calibration(self.h, int(seq), C.byref(cal)), "vio_set_calibration")
        self._cal_in[int(seq)] = _copy_fields(Calibration(), cal)

    def calibration(self, seq=0):
        """vio_get_calibration: the calibration in effect (ric re-orthonormalised; I / 0 on estimate_extrinsic = 2 handles)"""
        k = Calibration()
        self._chk(self.L.vio_get_calibration(self.h, int(seq), C.byref(k)), "vio_get_calibration")
        return k

    def set_camera(self, seq, cam):
        """vio_set_camera: slot seq gets its own camera model (a Camera) and restarts like a fresh handle; PINHOLE also sets the
        calibration's fx..p2"""
        if not isinstance(cam, Camera):
            raise TypeError("set_camera takes a Camera")
        self._chk(self.L.vio_set_camera(self.h, int(seq), C.byref(cam)), "vio_set_camera")
        if int(cam.model) == CAMERA_PINHOLE:
            for i, n in enumerate(CAMERA_PARAMS[CAMERA_PINHOLE]):
                setattr(self._cal_in[int(seq)], n, float(cam.p[i]))

    def camera(self, seq=0):
        """vio_get_camera: the slot's camera model (PINHOLE: the calibration's fx..p2)"""
        k = Camera()
        self._chk(self.L.vio_get_camera(self.h, int(seq), C.byref(k)), "vio_get_camera")
        return k

    def snapshot_bytes(self, seq):
        """vio_snapshot_bytes: bytes save([seq]) would produce for the slot right now"""
        n = int(self.L.vio_snapshot_bytes(self.h, int(seq)))
        if n < 0:
            raise VioError("vio_snapshot_bytes failed (%d): %s" % (n, self.L.vio_last_error().decode()))
        return n

    def save(self, seqs, out=None):
        """vio_save_seqs: one snapshot blob (uint8 array) per slot of seqs.  The handle is only read: it continues as if save had not been
        called.  The blobs are views into ONE buffer, packed back to back, so the device part leaves in a single copy; out = an optional
        uint8 buffer to pack them into (for instance PinnedArray(...).a), large enough for sum(snapshot_bytes)."""
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        n = len(seqs)
        if any(not 0 <= int(s) < self.S for s in seqs):
            raise VioError("vio_save_seqs failed (%d): seq out of range" % VIO_EINVAL)
        sizes = np.array([self.snapshot_bytes(int(s)) for s in seqs], np.int64)
        offs = np.zeros(n, np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        total = int(sizes.sum())
        buf = np.empty(total, np.uint8) if out is None else out
        if buf.dtype != np.uint8 or buf.ndim != 1 or buf.size < total or not buf.flags.c_contiguous:
            raise ValueError("save: out must be a contiguous uint8 buffer of at least %d bytes" % total)
        wrote = np.zeros(n, np.int64)
        self._chk(self.L.vio_save_seqs(self.h, n, seqs.ctypes.data, buf.ctypes.data, offs.ctypes.data, sizes.ctypes.data, wrote.ctypes.data),
                  "vio_save_seqs")
        return [buf[int(o):int(o) + int(w)] for o, w in zip(offs, wrote)]

    def load(self, seqs, blobs):
        """vio_load_seqs: restores blobs[i] (uint8 array or bytes, from save() of any handle with the same shape key and tracker lag) into
        slot seqs[i]; slots must be distinct.  Refused with VioError (every slot untouched) when a blob does not fit this handle."""
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        arrs = [np.ascontiguousarray(np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else b, np.uint8).reshape(-1)
                for b in blobs]
        if len(arrs) != len(seqs):
            raise ValueError("load: one blob per slot")
        sizes = np.array([a.size for a in arrs], np.int64)
        offs = np.zeros(len(arrs), np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        # blobs that are consecutive views of one buffer (what save() returns) go as they lie; others are packed back to back first
        base = arrs[0].ctypes.data if arrs else 0
        if all(a.ctypes.data == base + int(o) for a, o in zip(arrs, offs)):
            src_ptr, keep = base, arrs
        else:
            keep = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
            src_ptr = keep.ctypes.data
        self._chk(self.L.vio_load_seqs(self.h, len(seqs), seqs.ctypes.data, src_ptr, offs.ctypes.data, sizes.ctypes.data), "vio_load_seqs")
        for s in seqs:   # config_of() now describes the restored rig (the calibration in effect: ric is a rotation already)
            self._cal_in[int(s)] = _copy_fields(Calibration(), self.calibration(int(s)))

    def snapshot_layout(self):
        """The layout table of the handle: [(name, kind: 1 state / 0 scratch / 2 handle-wide, bytes per sequence, offset
        inside a blob's device part or -1)]"""
        out, i = [], 0
        name, kind, nb, off = C.create_string_buffer(64), C.c_int32(), C.c_int64(), C.c_int64()
        while i < self.L.vio_debug_snapshot_layout(self.h, i, name, C.byref(kind), C.byref(nb), C.byref(off)):
            out.append((name.value.decode(), int(kind.value), int(nb.value), int(off.value)))
            i += 1
        return out

    def config_of(self, seq):
        """The handle's configuration with slot seq's calibration merged in: what a one-sequence handle, the oracle or posegraph needs to
        compute what this slot computes"""
        if not 0 <= int(seq) < self.S:
            raise IndexError("seq out of range")
        return config_with_calibration(self.cfg, self._cal_in[int(seq)])

    @property
    def device(self):
        return int(self.L.vio_get_device(self.h))

    def host_buffers_done(self, calls_ago=0):
        """vio_host_buffers_done: have the page-locked image buffers of the feed issued `calls_ago` feeds ago been uploaded?"""
        return self._chk(self.L.vio_host_buffers_done(self.h, int(calls_ago)), "vio_host_buffers_done") == 1

    def close(self):
        if self.h:
            self.L.vio_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise VioError("%s failed (%d): %s" % (what, rc, self.L.vio_last_error().decode()))
        return rc

    def push_imu(self, seq, t, acc, gyr):
        t = np.ascontiguousarray(t, np.float64).reshape(-1)
        acc = np.ascontiguousarray(acc, np.float64).reshape(-1, 3)
        gyr = np.ascontiguousarray(gyr, np.float64).reshape(-1, 3)
        self._chk(self.L.vio_push_imu(self.h, seq, len(t), t.ctypes.data, acc.ctypes.data, gyr.ctypes.data), "vio_push_imu")

    def push_imu_batch(self, t, acc, gyr, n=None):
        """vio_push_imu_batch: t [S][stride], acc / gyr [S][stride][3]; n = optional per-sequence counts."""
        t = np.ascontiguousarray(t, np.float64).reshape(self.S, -1)
        stride = t.shape[1]
        acc = np.ascontiguousarray(acc, np.float64).reshape(self.S, stride, 3)
        gyr = np.ascontiguousarray(gyr, np.float64).reshape(self.S, stride, 3)
        nn = None if n is None else np.ascontiguousarray(n, np.int32).reshape(self.S)
        self._chk(self.L.vio_push_imu_batch(self.h, None if nn is None else nn.ctypes.data, stride, t.ctypes.data, acc.ctypes.data,
                                            gyr.ctypes.data), "vio_push_imu_batch")

    def feed(self, gray, depth, stamps, on_device=False, modes=None):
        stamps = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        assert len(stamps) == self.S
        m = None if modes is None else np.ascontiguousarray(modes, np.uint8).reshape(self.S)
        self._chk(self.L.vio_feed_modes(self.h, _ptr(gray), _ptr(depth), stamps.ctypes.data, None if m is None else m.ctypes.data,
                                        1 if on_device else 0), "vio_feed")
        self._keep = (gray, depth, stamps, m)   # host buffers stay alive until the next feed has returned (vio_abi.h)

    def track(self, gray, stamps, publish=True, on_device=False, modes=None, R_rel=None):
        """vio_track / vio_track_ex: modes = per-sequence FRAME_* (default: publish for all), R_rel = caller-supplied relative
        rotations [S][3][3] (rows of NaN = predict on the device)."""
        stamps = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        if modes is None and R_rel is None:
            self._keep = (gray, stamps)
            self._chk(self.L.vio_track(self.h, _ptr(gray), stamps.ctypes.data, 1 if publish else 0, 1 if on_device else 0), "vio_track")
            return
        m = np.full(self.S, FRAME_PUBLISH if publish else FRAME_TRACK, np.uint8) if modes is None else \
            np.ascontiguousarray(modes, np.uint8).reshape(self.S)
        R = None if R_rel is None else np.ascontiguousarray(R_rel, np.float64).reshape(self.S, 9)
        self._keep = (gray, stamps, m, R)
        self._chk(self.L.vio_track_ex(self.h, _ptr(gray), stamps.ctypes.data, m.ctypes.data, None if R is None else R.ctypes.data,
                                      1 if on_device else 0), "vio_track_ex")

    def predict_motion(self, seq, t0, t1):
        R = np.zeros(9)
        self._chk(self.L.vio_predict_motion(self.h, seq, float(t0), float(t1), R.ctypes.data), "vio_predict_motion")
        return R.reshape(3, 3)

    def process(self, depth, on_device=False):
        self._keep2 = depth
        self._chk(self.L.vio_process(self.h, _ptr(depth), 1 if on_device else 0), "vio_process")

    def process_obs(self, seq, ids, obs, depth, stamp):
        """Estimator::processImage(image, header) with a caller-supplied feature map (ids ascending, obs [n][7])."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 7)
        depth = np.ascontiguousarray(depth, np.uint16)
        self._keep3 = (ids, obs, depth)
        self._chk(self.L.vio_process_obs(self.h, seq, len(ids), ids.ctypes.data, obs.ctypes.data, depth.ctypes.data, float(stamp)),
                  "vio_process_obs")

    def process_obs_batch(self, n_obs, ids, obs, depth, stamps, on_device=False):
        n_obs = np.ascontiguousarray(n_obs, np.int32).reshape(self.S)
        ids = np.ascontiguousarray(ids, np.int32).reshape(self.S, -1)
        cap = ids.shape[1]
        obs = np.ascontiguousarray(obs, np.float64).reshape(self.S, cap, 7)
        stamps = np.ascontiguousarray(stamps, np.float64).reshape(self.S)
        self._keep3 = (n_obs, ids, obs, depth, stamps)
        self._chk(self.L.vio_process_obs_batch(self.h, n_obs.ctypes.data, ids.ctypes.data, obs.ctypes.data, cap, _ptr(depth),
                                               stamps.ctypes.data, 1 if on_device else 0), "vio_process_obs_batch")

    def packaged(self, seq=0, cap=2048):
        """The feature map packaged by the last track / feed (what the nodelet pushes to feature_buf): ids, obs [n][7]."""
        ids, obs = np.zeros(cap, np.int32), np.zeros((cap, 7))
        n = self._chk(self.L.vio_get_packaged(self.h, seq, cap, ids.ctypes.data, obs.ctypes.data), "vio_get_packaged")
        return ids[:n].copy(), obs[:n].copy()

    def solver_kind(self):
        """0 persistent fallback kernel, 1 phased solver (LDS-resident Schur complement), 2 phased solver (HBM-resident, large windows)"""
        self.L.vio_get_solver_kind.argtypes = [C.c_void_p]
        return self.L.vio_get_solver_kind(self.h)

    def bound_stats(self, seq=0):
        """(inverse depths cut by the upper bound, bounded landmarks that entered solves, line-search trial evaluations, shortened steps) of
        sequence seq since creation (estimator.cpp:1282-1297; Ceres' projected Armijo line search on the bounds-constrained program)"""
        o = np.zeros(4, np.int64)
        self.L.vio_get_bound_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._chk(self.L.vio_get_bound_stats(self.h, int(seq), o.ctypes.data), "vio_get_bound_stats")
        return tuple(int(x) for x in o)

    def preint_ahead_stats(self, per_seq=False):
        """(used, declined): frames for which be_ingest took over the IMU pre-integration computed ahead of it (VIO_PREINT_AHEAD) / was handed
        one but integrated itself, summed over the sequences since creation; per_seq=True: an [S][2] array instead.  Waits for the handle."""
        o, ps = np.zeros(2, np.int64), np.zeros((self.S, 2), np.int64)
        self.L.vio_debug_preint_ahead.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.L.vio_debug_preint_ahead(self.h, o.ctypes.data, ps.ctypes.data), "vio_debug_preint_ahead")
        return ps if per_seq else (int(o[0]), int(o[1]))

    def marg_split_stats(self, per_seq=False):
        """Marginalisations that ran as be_marg_pre + be_marg_alg (VIO_MARG_SPLIT) since creation, summed over the sequences; per_seq=True: an
        [S] array instead.  Waits for the handle."""
        o, ps = np.zeros(1, np.int64), np.zeros(self.S, np.int64)
        self.L.vio_debug_marg_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.L.vio_debug_marg_split(self.h, o.ctypes.data, ps.ctypes.data), "vio_debug_marg_split")
        return ps if per_seq else int(o[0])

    def ex_calibration(self, seq=0, history=False):
        """estimate_extrinsic = 2 (InitialEXRotation): dict(state = 2 calibrating / 1 calibrated / 0 not a mode-2 handle, pairs, success_frame
        (frames_processed after the frame that succeeded, -1 while calibrating), ric (3 x 3, current estimate), sv (4 singular values of the last
        averaging step)); with history=True also history = [pairs][3][4]: q(Rc), q(Rimu), q(Rc_g) (w x y z) of every stored pair, oldest first."""
        o = np.zeros(16, np.float64)
        hist = np.zeros((2048 if history else 0, 12), np.float64)
        n = self._chk(self.L.vio_get_ex_calibration(self.h, int(seq), o.ctypes.data, hist.shape[0], hist.ctypes.data if history else None),
                      "vio_get_ex_calibration")
        out = dict(state=int(o[0]), pairs=int(o[1]), success_frame=int(o[2]), ric=o[3:12].reshape(3, 3).copy(), sv=o[12:16].copy())
        if history:
            out["history"] = hist[:min(n, hist.shape[0])].reshape(-1, 3, 4).copy()
        return out

    def marg_certificate(self, seq=0):
        """marg_exact = 2: (marginalisations whose certificate failed since creation, last one certified?)"""
        o = np.zeros(2, np.int32)
        self.L.vio_get_marg_certificate.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._chk(self.L.vio_get_marg_certificate(self.h, int(seq), o.ctypes.data), "vio_get_marg_certificate")
        return int(o[0]), bool(o[1])

    def capacity(self):
        c = np.zeros(3, np.int32)
        self._chk(self.L.vio_get_capacity(self.h, c.ctypes.data), "vio_get_capacity")
        return dict(tracks=int(c[0]), landmarks=int(c[1]), imu=int(c[2]))

    def reset_seq(self, seq):
        """Estimator::clearState() + setParameter() for one sequence (the nodelet's stream-discontinuity restart: the tracker is kept)"""
        self._chk(self.L.vio_reset_seq(self.h, seq), "vio_reset_seq")

    def reset_tracker_seq(self, seq):
        self._chk(self.L.vio_reset_tracker_seq(self.h, seq), "vio_reset_tracker_seq")

    def sync(self):
        self._chk(self.L.vio_sync(self.h), "vio_sync")

    def reset(self):
        self._chk(self.L.vio_reset(self.h), "vio_reset")

    def stream(self):
        return self.L.vio_get_stream(self.h)

    def status(self, seq=0):
        s = Status()
        self._chk(self.L.vio_get_status(self.h, seq, C.byref(s)), "vio_get_status")
        return s

    def status_all(self):
        """vio_status of every sequence (two device reads for the whole batch)"""
        arr = (Status * self.S)()
        self._chk(self.L.vio_get_status_all(self.h, arr), "vio_get_status_all")
        return list(arr)

    def window(self, seq=0):
        w = np.zeros((self.W + 1, 17))
        self._chk(self.L.vio_get_window(self.h, seq, w.ctypes.data), "vio_get_window")
        return w

    def odometry(self):
        o = np.zeros((self.S, 11))
        self._chk(self.L.vio_get_odometry(self.h, o.ctypes.data), "vio_get_odometry")
        return o

    def odometry_history(self, seq=0, cap=2048):
        o = np.zeros((cap, 11))
        n = self._chk(self.L.vio_get_odometry_history(self.h, seq, cap, o.ctypes.data), "vio_get_odometry_history")
        return o[:min(n, cap)]

    def set_tracker_lag(self, lag):
        """0: the tracker of frame f+1 waits for the optimisation of frame f; 1: it overlaps it, reading latest_Bg / td as of frame f-1"""
        self._chk(self.L.vio_set_tracker_lag(self.h, int(lag)), "vio_set_tracker_lag")

    def set_fisheye_mask(self, mask):
        """FISHEYE: the feature mask starts from `mask` (H x W u8, 255 = usable) instead of all 255 (feature_tracker.cpp:175-176); None = off"""
        if mask is None:
            self._chk(self.L.vio_set_fisheye_mask(self.h, None, 0), "vio_set_fisheye_mask")
            return
        on_dev = hasattr(mask, "data_ptr") and getattr(mask, "is_cuda", False)
        m = mask if on_dev else np.ascontiguousarray(mask, np.uint8)
        if not on_dev and m.shape != (self.cfg.height, self.cfg.width):
            raise ValueError("fisheye mask must be height x width")
        self._chk(self.L.vio_set_fisheye_mask(self.h, _ptr(m), 1 if on_dev else 0), "vio_set_fisheye_mask")

    def latest_odometry(self, seq=0):
        """IMU-rate pose (pubLatestOdometry): t, P(3), Q(wxyz), V(3) of the newest window state propagated through the IMU pushed since"""
        o = np.zeros(11)
        self._chk(self.L.vio_get_latest_odometry(self.h, seq, o.ctypes.data), "vio_get_latest_odometry")
        return o

    def latest_odometry_all(self, out=None):
        """latest_odometry of every sequence in one launch and one copy: [S, 11].  out = a device address (DeviceBuffer.ptr, a torch tensor)
        that receives the rows instead; nothing is returned then."""
        if out is not None:
            self._chk(self.L.vio_get_latest_odometry_all(self.h, _ptr(out), 1), "vio_get_latest_odometry_all")
            return None
        o = np.zeros((self.S, 11))
        self._chk(self.L.vio_get_latest_odometry_all(self.h, o.ctypes.data, 0), "vio_get_latest_odometry_all")
        return o

    def imu_rate_odometry(self, since=None, cap=256, out=None):
        """The pose after every IMU sample newer than the window state, for every sequence (what pubLatestOdometry publishes, one row per
        sample): (n_rows [S], rows [S, cap, 11]).  rows[s, :min(n_rows[s], cap)] are t, P(3), Q(wxyz), V(3) in time order, the rest is
        zero; n_rows may exceed cap.  since = [S] stamps: only rows with t > since[s] (a poller passes the last stamp it received).
        out = a device address that receives [S][cap][11] instead: only n_rows is returned then.  cap = 0 only counts."""
        cap = int(cap)
        n = np.zeros(self.S, np.int32)
        sn = None if since is None else np.ascontiguousarray(since, np.float64).reshape(self.S)
        sp = None if sn is None else sn.ctypes.data
        if out is not None:
            self._chk(self.L.vio_get_imu_rate_odometry(self.h, sp, cap, n.ctypes.data, _ptr(out), 1), "vio_get_imu_rate_odometry")
            return n
        rows = np.zeros((self.S, max(cap, 0), 11))
        self._chk(self.L.vio_get_imu_rate_odometry(self.h, sp, cap, n.ctypes.data, rows.ctypes.data if cap > 0 else None, 0),
                  "vio_get_imu_rate_odometry")
        return n, rows

    def publish(self, cap=None, on_device=False, lists=(True, True, True), fill=0.0):
        """pubPointCloud and pubKeyframe of every sequence in one launch and one copy (vio_publish_all): dict(counts [S, 4] = n_cloud, n_margin,
        n_kf, kf_valid; kf_pose [S, 8] = stamp, P(3), Q(wxyz) of window frame W-2; cloud [S, cap, 3]; margin [S, cap, 3]; kf_points [S, cap, 8] =
        world point, x, y, u, v, feature id).  Rows beyond min(count, cap), and kf_pose where kf_valid is 0, hold `fill`; the counts may
        exceed cap.  cap = None: the landmark capacity, so nothing is cut.  lists[i] = False: that list is only counted (None is returned for
        it).  on_device = True: the rows and poses stay in HBM, in DeviceBuffers returned under the same keys."""
        cap = self.capacity()["landmarks"] if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must be >= 0")
        if len(lists) != 3:
            raise ValueError("lists = (cloud, margin, kf_points)")
        S = self.S
        counts = np.zeros((S, 4), np.int32)
        names, widths = ("cloud", "margin", "kf_points"), (3, 3, 8)
        if on_device:
            pose = DeviceBuffer(S * 8 * 8)
            pose.upload(0, np.full((S, 8), float(fill)))
            bufs = []
            for w, on in zip(widths, lists):
                bufs.append(DeviceBuffer(max(S * cap * w, 1) * 8) if on else None)
                if on and cap > 0:
                    bufs[-1].upload(0, np.full((S, cap, w), float(fill)))
            self._chk(self.L.vio_publish_all(self.h, cap, counts.ctypes.data, pose.ptr, *[None if b is None else b.ptr for b in bufs], 1),
                      "vio_publish_all")
            return dict(zip(("counts", "kf_pose") + names, [counts, pose] + bufs))
        pose = np.full((S, 8), float(fill))
        out = [np.full((S, cap, w), float(fill)) if on else None for w, on in zip(widths, lists)]
        self._chk(self.L.vio_publish_all(self.h, cap, counts.ctypes.data, pose.ctypes.data, *[_ptr(o) for o in out], 0), "vio_publish_all")
        return dict(zip(("counts", "kf_pose") + names, [counts, pose] + out))

    def set_relo_frame(self, seq, stamp, index, match_points, relo_t, relo_r):
        """Estimator::setReloFrame (estimator.cpp:1728-1747): match_points[n][3] = (x, y, feature id) ascending in id"""
        mp = np.ascontiguousarray(match_points, np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(relo_t, np.float64).reshape(3)
        R = np.ascontiguousarray(relo_r, np.float64).reshape(9)
        self._chk(self.L.vio_set_relo_frame(self.h, seq, float(stamp), int(index), len(mp), mp.ctypes.data, t.ctypes.data, R.ctypes.data), "vio_set_relo_frame")

    def relo(self, seq=0):
        o = np.zeros(30)
        self._chk(self.L.vio_get_relo(self.h, seq, o.ctypes.data), "vio_get_relo")
        return dict(relative_t=o[0:3], relative_q=o[3:7], relative_yaw=o[7], drift_t=o[8:11], drift_r=o[11:20].reshape(3, 3), relo_pose=o[20:27],
                    pending=int(o[27]), local_index=int(o[28]), n_factors=int(o[29]))

    def extrinsic(self, seq=0):
        e = np.zeros(13)
        self._chk(self.L.vio_get_extrinsic(self.h, seq, e.ctypes.data), "vio_get_extrinsic")
        return e

    def tracks(self, seq=0, cap=2048):
        ids, cnt = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        cur, un, vel = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        n = self._chk(self.L.vio_get_tracks(self.h, seq, cap, ids.ctypes.data, cnt.ctypes.data, cur.ctypes.data, un.ctypes.data,
                                            vel.ctypes.data), "vio_get_tracks")
        return ids[:n], cnt[:n], cur[:n], un[:n], vel[:n]

    def landmarks(self, seq=0, cap=4096):
        out = np.zeros((cap, 7))
        n = self._chk(self.L.vio_get_landmarks(self.h, seq, cap, out.ctypes.data), "vio_get_landmarks")
        return out[:min(n, cap)]

    def landmarks_ex(self, seq=0, cap=4096):
        out = np.zeros((cap, 12))
        n = self._chk(self.L.vio_get_landmarks_ex(self.h, seq, cap, out.ctypes.data), "vio_get_landmarks_ex")
        return out[:min(n, cap)]

    def prior(self, seq=0):
        n = 6 * self.W + 16
        J, r, x0, pres = np.zeros((n, n)), np.zeros(n), np.zeros(self.W * 7 + 17), np.zeros(self.W + 3, np.uint8)
        k = self._chk(self.L.vio_get_prior(self.h, seq, J.ctypes.data, r.ctypes.data, x0.ctypes.data, pres.ctypes.data), "vio_get_prior")
        return (J, r, x0, pres) if k else None

    def marg_stage_set(self, seq, st, _fn="vio_debug_marg_set"):
        """vio_debug_marg_set: stage one sequence's pre-marginalisation state (include/vio_abi.h vio_marg_stage_in).  st: dict of lm_order [n_lm]
        (n_lm may be given on its own), lm_id, lm_start, lm_nobs, lm_solve_flag, lm_dyn, lm_est_flag [NL], lm_depth [NL], lm_obs [NL, W+1, 9], Ps, Vs,
        Bas, Bgs [W+1, 3], Rs [W+1, 3, 3], Headers [W+1], ric [3, 3], tic, g [3], td, ring_base, marginalization_flag, pre_idx [W+1], prior = None or
        dict(present [W+3], H [n, n], r [n], x0 [7 W + 17]), and on use_imu handles imu_n [W+1], imu_dt [W+1, 64], imu_acc / imu_gyr [W+1, 64, 3],
        imu_acc0 / imu_gyr0 / imu_ba / imu_bg [W+1, 3].  Array SIZES are checked here; the values are the library's to refuse (VioError)."""
        W, NL, n = self.W, self.capacity()["landmarks"], 6 * self.W + 16
        keep, s = [], MargStageIn()

        def arr(a, dtype, size, name):
            a = np.ascontiguousarray(a, dtype).reshape(-1)
            if a.size != size:
                raise ValueError("%s holds %d values, expected %d" % (name, a.size, size))
            keep.append(a)
            return a.ctypes.data
        order = np.zeros(NL, np.int32)
        lo = np.asarray(st["lm_order"], np.int32).reshape(-1)
        if lo.size > NL:
            raise ValueError("lm_order holds more than NL entries")
        order[:lo.size] = lo
        s.t.lm_order = arr(order, np.int32, NL, "lm_order")
        for name in _PUBLISH_INT[1:]:
            setattr(s.t, name, arr(st[name], np.int32, NL, name))
        sizes = dict(lm_depth=NL, lm_obs=NL * (W + 1) * 9, Ps=3 * (W + 1), Rs=9 * (W + 1), Headers=W + 1, ric=9, tic=3)
        for name in _PUBLISH_F64:
            setattr(s.t, name, arr(st[name], np.float64, sizes[name], name))
        s.lm_est_flag = arr(st["lm_est_flag"], np.int32, NL, "lm_est_flag")
        s.n_lm, s.ring_base, s.marginalization_flag = int(st.get("n_lm", lo.size)), int(st["ring_base"]), int(st["marginalization_flag"])
        for name in ("Vs", "Bas", "Bgs"):
            setattr(s, name, arr(st[name], np.float64, 3 * (W + 1), name))
        s.g, s.td = arr(st["g"], np.float64, 3, "g"), float(st["td"])
        pr = st.get("prior")
        s.has_prior = int(st.get("has_prior", pr is not None))
        if pr is not None:
            s.prior_present = arr(pr["present"], np.int32, W + 3, "prior present")
            s.prior_H, s.prior_r = arr(pr["H"], np.float64, n * n, "prior H"), arr(pr["r"], np.float64, n, "prior r")
            s.prior_x0 = arr(pr["x0"], np.float64, 7 * W + 17, "prior x0")
        s.pre_idx = arr(st["pre_idx"], np.int32, W + 1, "pre_idx")
        if "imu_n" in st:
            s.imu_n = arr(st["imu_n"], np.int32, W + 1, "imu_n")
            s.imu_dt = arr(st["imu_dt"], np.float64, (W + 1) * 64, "imu_dt")
            for name in ("imu_acc", "imu_gyr"):
                setattr(s, name, arr(st[name], np.float64, (W + 1) * 64 * 3, name))
            for name in ("imu_acc0", "imu_gyr0", "imu_ba", "imu_bg"):
                setattr(s, name, arr(st[name], np.float64, (W + 1) * 3, name))
        fn = getattr(self.L, _fn)
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(MargStageIn)]
        self._chk(fn(self.h, int(seq), C.byref(s)), _fn)

    def marg_stage_run(self):
        """vio_debug_marg_run: the marginalisation launches of vio_feed for this handle, then a wait"""
        self.L.vio_debug_marg_run.argtypes = [C.c_void_p]
        self._chk(self.L.vio_debug_marg_run(self.h), "vio_debug_marg_run")

    def marg_stage_get(self, seq):
        """vio_debug_marg_get: dict of prior_H [n, n], prior_r, prior_x0, prior_present, prior_c0, has_prior, dbg [5], hbm (the handle runs
        be_marg_hbm_kernel) and then margA [15 + n, 15 + n flat], margB, margV [n, n], b_r (NaN where the handle keeps them in LDS)."""
        W, n = self.W, 6 * self.W + 16
        mq = 15 + n
        o = dict(prior_H=np.full((n, n), np.nan), prior_r=np.full(n, np.nan), prior_x0=np.full(7 * W + 17, np.nan),
                 prior_present=np.full(W + 3, -1, np.int32), prior_c0=np.full(1, np.nan), has_prior=np.full(1, -1, np.int32),
                 dbg5=np.full(5, -1, np.int32), margA=np.full(mq * mq, np.nan), margB=np.full(mq, np.nan), margV=np.full((n, n), np.nan),
                 b_r=np.full(n, np.nan), hbm_valid=np.full(1, -1, np.int32))
        s = MargStageOut()
        for name, a in o.items():
            setattr(s, name, a.ctypes.data)
        self.L.vio_debug_marg_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(MargStageOut)]
        self._chk(self.L.vio_debug_marg_get(self.h, int(seq), C.byref(s)), "vio_debug_marg_get")
        o["prior_c0"], o["has_prior"], o["hbm"] = float(o["prior_c0"][0]), int(o["has_prior"][0]), bool(o.pop("hbm_valid")[0])
        o["dbg"] = o.pop("dbg5")
        return o

    def solve_stage_set(self, seq, st):
        """vio_debug_solve_set: the state of marg_stage_set (same dict), staged in front of a solve"""
        self.marg_stage_set(seq, st, _fn="vio_debug_solve_set")

    def solve_stage_run(self, slots=-1, stop="none", radius0=0.0):
        """vio_debug_solve_run: ps_setup, `slots` whole slots and the next one up to `stop` (a key of SOLVE_STOP), then a wait; slots < 0: the
        whole solve with ps_final, as vio_feed launches it"""
        self.L.vio_debug_solve_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
        self._chk(self.L.vio_debug_solve_run(self.h, int(slots), SOLVE_STOP[stop], float(radius0)), "vio_debug_solve_run")

    def solve_stage_get(self, seq):
        """vio_debug_solve_get: dict of the SolveSt scalars by name (stage as a name of PS_STAGES), X / Xc = dict(pose [W+1, 7], sb [W+1, 9], ex [7],
        td), feat / cfeat [F], var_slots [Fa], H [P, P], g, sp [P], Hpl [Fa, P], Hll, gl, sl [Fa], Sc [LW, LW] (lower tiles), dgp / gnp / stp [P],
        dgl / gnl / stl [Fa]; which of them mean what after which stop phase: include/vio_abi.h"""
        W1, NL = self.W + 1, self.capacity()["landmarks"]
        Pn = 15 * W1 + 7
        LW = (Pn + 15) & ~15
        o = dict(scal_i=np.full(11, -1, np.int32), scal_d=np.full(7, np.nan), X=np.full(16 * W1 + 8, np.nan), Xc=np.full(16 * W1 + 8, np.nan),
                 feat=np.full(NL, np.nan), cfeat=np.full(NL, np.nan), var_slots=np.full(NL, -1, np.int32), H=np.full((Pn, Pn), np.nan),
                 g=np.full(Pn, np.nan), sp=np.full(Pn, np.nan), Hpl=np.full((NL, Pn), np.nan), Hll=np.full(NL, np.nan), gl=np.full(NL, np.nan),
                 sl=np.full(NL, np.nan), Sc=np.full((LW, LW), np.nan), dgp=np.full(Pn, np.nan), dgl=np.full(NL, np.nan), gnp=np.full(Pn, np.nan),
                 gnl=np.full(NL, np.nan), stp=np.full(Pn, np.nan), stl=np.full(NL, np.nan))
        s = SolveStageOut()
        for name, a in o.items():
            setattr(s, name, a.ctypes.data)
        self.L.vio_debug_solve_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(SolveStageOut)]
        self._chk(self.L.vio_debug_solve_get(self.h, int(seq), C.byref(s)), "vio_debug_solve_get")
        o.update(zip(_SOLVE_SCAL_I, (int(v) for v in o.pop("scal_i"))))
        o.update(zip(_SOLVE_SCAL_D, (float(v) for v in o.pop("scal_d"))))
        o["stage"] = PS_STAGES[o["stage"]]
        for k in ("X", "Xc"):
            v = o[k]
            o[k] = dict(pose=v[:7 * W1].reshape(W1, 7).copy(), sb=v[7 * W1:16 * W1].reshape(W1, 9).copy(), ex=v[16 * W1:16 * W1 + 7].copy(),
                        td=float(v[16 * W1 + 7]))
        F, Fa = o["F"], o["Fa"]
        for k in ("feat", "cfeat"):
            o[k] = o[k][:F].copy()
        for k in ("var_slots", "Hpl", "Hll", "gl", "sl", "dgl", "gnl", "stl"):
            o[k] = o[k][:Fa].copy()
        return o

    KERNELS = ("fe_begin", "fe_pyrdown", "fe_predict", "fe_lk", "fe_select", "fe_fast", "fe_add", "be_ingest", "be_solve", "be_marg")

    def profile_begin(self, max_steps):
        self._chk(self.L.vio_profile_begin(self.h, max_steps), "vio_profile_begin")

    def profile_end(self):
        t = np.zeros(len(self.KERNELS))
        n = self._chk(self.L.vio_profile_end(self.h, len(t), t.ctypes.data), "vio_profile_end")
        return n, dict(zip(self.KERNELS, t.tolist()))

    def timings(self):
        t = np.zeros(8)
        n = self._chk(self.L.vio_get_timings(self.h, 8, t.ctypes.data), "vio_get_timings")
        return t[:n]


# ------------------------------------------------------------------------------------------------ reference-shaped mirrors
class FeatureTracker:
    """FeatureTracker (feature_tracker.h:31-97) backed by one HBM-resident sequence."""

    def __init__(self, batch, seq=0):
        self.b, self.seq = batch, seq
        self.ids = self.track_cnt = self.cur_pts = self.cur_un_pts = self.pts_velocity = None

    def readImage(self, img, cur_time, relative_R=None, publish=True):
        """readImage(const cv::Mat&, double, const Matrix3d& relative_R = Identity) (feature_tracker.h:36-37); publish is the
        global PUB_THIS_FRAME.  relative_R=None predicts it on the device from the pushed IMU (Estimator::predictMotion)."""
        assert self.b.S == 1, "the per-sequence mirror drives single-sequence batches"
        R = None if relative_R is None else np.asarray(relative_R, np.float64).reshape(1, 9)
        self.b.track(np.ascontiguousarray(img, np.uint8), [cur_time], publish=publish, R_rel=R)
        self.ids, self.track_cnt, self.cur_pts, self.cur_un_pts, self.pts_velocity = self.b.tracks(self.seq)

    def updateID(self, i):
        """ids are assigned on the device inside readImage; kept for call-site compatibility (estimator_nodelet.cpp:324-330)."""
        return i < len(self.ids)

    def image_map(self):
        """The feature map of estimator_nodelet.cpp:336-363 for the last published frame: {feature_id: (x, y, 1, u, v, vx, vy)}."""
        ids, obs = self.b.packaged(self.seq)
        return {int(i): o for i, o in zip(ids, obs)}


class Estimator:
    """Estimator (estimator.h:25-201) call surface backed by one HBM-resident sequence."""

    def __init__(self, cfg=None, imu_capacity=8192):
        self.batch = VioBatch(cfg, 1, imu_capacity)
        self.featureTracker = FeatureTracker(self.batch)

    def inputIMU(self, t, linearAcceleration, angularVelocity):
        self.batch.push_imu(0, [t], [linearAcceleration], [angularVelocity])

    def predictMotion(self, t0, t1):
        """Matrix3d predictMotion(double t0, double t1) (estimator.h:56, estimator.cpp:1790-1860)."""
        return self.batch.predict_motion(0, t0, t1)

    def processImage(self, image, header, depth_mm):
        """processImage(const map<int, Matrix<double,7,1>>& image, const Header& header) (estimator.h:46) preceded by
        f_manager.inputDepth(depth) (estimator_nodelet.cpp:537-539).  image: {feature_id: 7-vector}; header: stamp in seconds."""
        ids = sorted(image)
        obs = np.array([image[i] for i in ids], np.float64).reshape(-1, 7)
        self.batch.process_obs(0, ids, obs, depth_mm, header)
        return self.batch.status(0).code

    def processLastTracked(self, depth_mm):
        """Short cut without the host round trip: inputDepth + processImage on the map the last readImage packaged on the device."""
        self.batch.process(np.ascontiguousarray(depth_mm, np.uint16))
        return self.batch.status(0).code

    def clearState(self):
        """Estimator::clearState() (estimator.cpp:43-116): the estimator side only, the FeatureTracker keeps its state"""
        self.batch.reset_seq(0)

    def setParameter(self):
        """estimator.cpp:15-41: parameters are bound at construction (vio_reset_seq re-applies them)"""

    @property
    def solver_flag(self):
        return self.batch.status(0).solver_flag

    def window(self):
        return self.batch.window(0)
