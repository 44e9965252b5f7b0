/* MI355X-native VIO hot path — C ABI (the drop-in boundary).
 *
 * The reference has no FFI layer: its boundary is the public member-function surface of FeatureTracker / Estimator /
 * FeatureManager plus mutable globals (vins_estimator/src/utility/parameters.h:17-79).  Each entry point below names
 * the reference interface it replaces.  A handle owns a *batch* of S independent sequences (S = 1 reproduces the
 * reference's one-Estimator-per-process use); all state lives in HBM behind the handle, configuration is per handle
 * instead of process-global.  Plain C types only; the caller owns input buffers for the duration of a call.
 *
 * Host buffers: every entry point that takes host memory (images with on_device == 0, stamps, modes, R_rel, feature maps) enqueues
 * asynchronous uploads.  From pageable memory the runtime stages the copy before the call returns; from page-locked memory
 * (vio_host_alloc) the copy is truly asynchronous: such buffers must stay untouched until the NEXT call on the handle that takes host
 * buffers, any getter, or vio_sync has returned (those calls wait for the pending uploads first).  Exception (round 5): the IMAGES handed to
 * vio_feed / vio_feed_modes keep TWO uploads in flight -- they are free when vio_host_buffers_done(h, calls_ago) returns 1, and at the latest
 * when the second next vio_feed THAT TAKES HOST IMAGES, any getter or vio_sync has returned (rotate three page-locked image sets, or poll the
 * query; feeds of device-resident frames in between do not count).  This is a BREAKING change against the round-4 contract ("free when the
 * next vio_feed has returned"): a caller that ping-pongs TWO page-locked image sets must move to three or poll.  vio_abi_version() tells the
 * contracts apart (>= 5: this one); VIO_UPLOADS_IN_FLIGHT=1 in the environment restores the old wait (one upload in flight, two sets suffice).
 *
 * Threading: a handle is not re-entrant.  vio_push_imu / vio_push_imu_batch may be called from another thread than
 * vio_track / vio_process / vio_feed (internal lock), mirroring Estimator::inputIMU being called from ROS callback threads
 * (estimator.cpp:1749-1766).  vio_last_error is thread-local: it reports the last failure of the CALLING thread.
 */
#ifndef VIO_ABI_H
#define VIO_ABI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* error conventions (reference: void everywhere, ROS_ASSERT aborts, busy-wait for IMU at estimator.cpp:178-183) */
enum {
    VIO_OK = 0,
    VIO_NEED_IMU = 1,   /* IMU not yet pushed through stamp + td; nothing was consumed, call again later */
    VIO_REBOOTED = 2,   /* failureDetection() fired (estimator.cpp:345-353); the sequence was reset */
    VIO_EINVAL = -1,
    VIO_EDEVICE = -2,   /* HIP error / no GPU: the product path never falls back to the CPU */
    VIO_ECAPACITY = -3
};

/* Replaces the globals read by the hot path (parameters.h:11-79) and config/realsense/vio.yaml keys. */
typedef struct vio_config {
    int32_t width, height;          /* COL, ROW                      image_width / image_height */
    int32_t max_cnt, min_dist;      /* MAX_CNT, MIN_DIST             max_cnt / min_dist */
    int32_t grid_rows, grid_cols;   /* NUM_GRID_ROWS / NUM_GRID_COLS */
    int32_t window_size;            /* WINDOW_SIZE (compile-time 10 upstream, parameters.h:12); 4..20 here */
    int32_t max_landmarks;          /* NUM_OF_F (parameters.h:14): capacity of the landmark table */
    int32_t fix_depth;              /* FIX_DEPTH */
    int32_t estimate_extrinsic;     /* ESTIMATE_EXTRINSIC: 0 fixed, 1 refined by the solver, 2 = no extrinsic: ric / tic are ignored (ric = I,
                                       tic = 0, parameters.cpp:181-190) and the rotation is calibrated online per sequence (InitialEXRotation,
                                       estimator.cpp:208-226; both initialisations wait for it), then refined as in mode 1: see
                                       vio_get_ex_calibration.  Mode 2 needs use_imu = 1. */
    int32_t estimate_td;            /* ESTIMATE_TD */
    int32_t max_iterations;         /* NUM_ITERATIONS  max_num_iterations */
    int32_t ransac_max_iters;       /* cv::findFundamentalMat RANSAC iteration cap (1000) */
    int32_t lk_max_level;           /* maxLevel of calcOpticalFlowPyrLK: 1 for the IMU-aided call (feature_tracker.cpp:303) */
    int32_t dynamic_init;           /* !STATIC_INIT (parameters.cpp:167): 0 = static initialisation (gyro-bias + optimisation on the
                                       IMU-propagated window, estimator.cpp:266-283), 1 = SfM + visual-inertial alignment
                                       (initialStructure, estimator.cpp:384-579) */
    int32_t use_imu;                /* USE_IMU (yaml key `imu`, parameters.cpp:148): 0 = visual odometry on RGB-D: no IMU factors, pose 0
                                       constant, initFramePoseByPnP per frame, LK maxLevel = lk_max_level (3 upstream) without prediction */
    int32_t reference_quirks;       /* bit 0 (VIO_QUIRK_LATEST_FRONT): vio_get_latest_odometry replays the buffered IMU the way
                                       Estimator::updateLatestStates does (estimator.cpp:1779-1786): every step uses the values of the queue's
                                       FRONT sample (the reference's behaviour).  0 = every sample with its own values. */
    int32_t marg_exact;             /* 1 = the marginalisation follows MarginalizationInfo::marginalize literally (marginalization_factor.cpp:
                                       281-315): eigen-decomposition of the FULL m x m marginalised block (pose 0, speed-bias 0 and every
                                       landmark that starts in frame 0) with the 1e-8 cut, then eigen-decomposition of the reduced system and the
                                       prior rebuilt from the truncated factors J = S^1/2 V^T, r = S^-1/2 V^T b.  0 (default) = the fast form
                                       (analytic landmark elimination, prior kept as a quadratic form; DESIGN.md deviations 10 / 13).
                                       2 (round 5) = the literal algorithm with a CERTIFIED first inverse: A_mm^+ = A_mm^-1 is formed by blocks
                                       (exact for the diagonal landmark block) and every frame proves lambda_min(A_mm) > 1e-7 from a bound on
                                       |A_mm^-1|_F, i.e. that the reference's 1e-8 cut could not have dropped anything; the second half (the
                                       new prior's eigen-decomposition with its cut, which does drop directions) is the literal one. */
    int32_t equalize;               /* EQUALIZE (yaml key `equalize`, parameters.cpp:110): 1 = cv::createCLAHE(3.0, Size(8, 8)) on every image
                                       before tracking (feature_tracker.cpp:269-275).  Occupies what used to be alignment padding: the
                                       offsets of all other fields are unchanged. */
    double fx, fy, cx, cy, k1, k2, p1, p2; /* pinhole projection_parameters / distortion_parameters */
    double focal_length;            /* FOCAL_LENGTH = 460 (parameters.h:11) */
    double f_threshold;             /* F_THRESHOLD */
    double depth_min, depth_max;    /* DEPTH_MIN_DIST / DEPTH_MAX_DIST */
    double acc_n, acc_w, gyr_n, gyr_w, g_norm;
    double ric[9];                  /* extrinsicRotation, row-major, imu<-cam */
    double tic[3];                  /* extrinsicTranslation */
    double td, tr;                  /* TD, TR */
    double min_parallax_px;         /* keyframe_parallax */
    double init_depth;              /* INIT_DEPTH = 5 (parameters.cpp:215) */
} vio_config;

enum { VIO_QUIRK_LATEST_FRONT = 1,
       /* bit 2 (value 4): ignored by the library; the test oracle mirrors deviation 15 (extrinsic held in a relocalisation solve) when set */
       VIO_ORACLE_RELO_HOLDS_EXTRINSIC = 4,
       /* bit 3 (value 8), TEST SWITCH, not a reference behaviour (both sides read it): the inverse-depth bound of depth-less landmarks
        * (estimator.cpp:1282-1297) is honoured by clamping candidates only, as rounds 1 - 5 did (former deviation 5).  0 = Ceres'
        * treatment of a bounds-constrained program: x0 projected before the first evaluation, projected Armijo line search along every
        * trust-region step (be_phased.h ps_eval; oracle/backend.cpp solve()). */
       VIO_QUIRK_BOUND_CLAMP_ONLY = 8,
       /* TEST HOOK, not a reference behaviour: bits 8..11 = n: the first n Cholesky factorisations of EVERY solve are reported as failed
        * (on both sides: the oracle reads the same bits), which walks the mu *= 10 retry ladder of the trust-region loop
        * (oracle/backend.cpp solve(); be_phased.h ps_serial).  Every retry uses one iteration slot: see VIO_EXTRA_SLOTS. */
       VIO_TEST_CHOL_FAIL_SHIFT = 8, VIO_TEST_CHOL_FAIL_MASK = 15 };

typedef struct vio_batch vio_batch; /* opaque */

/* Per-sequence calibration (ABI 10): the fields of vio_config that describe ONE sensor rig.  Every sequence of a handle has its own copy;
 * vio_create gives every slot vio_calibration_from_config(cfg), vio_set_calibration replaces one.  All other vio_config fields stay
 * handle-wide because they size buffers or select code paths: image size, grid, max_cnt, min_dist, window, landmark capacity, use_imu,
 * dynamic_init, estimate_extrinsic, estimate_td, marg_exact, equalize, fix_depth, focal_length (FOCAL_LENGTH is a constant upstream,
 * parameters.h:11), the depth range, thresholds and quirk bits. */
typedef struct vio_calibration {
    double fx, fy, cx, cy, k1, k2, p1, p2;   /* pinhole projection_parameters / distortion_parameters */
    double ric[9];                            /* extrinsicRotation imu<-cam, row-major: initial value (estimate_extrinsic 1) or fixed (0) */
    double tic[3];                            /* extrinsicTranslation */
    double td, tr;                            /* TD (initial value when estimate_td), TR (rolling_shutter_tr) */
    double acc_n, acc_w, gyr_n, gyr_w, g_norm;
} vio_calibration;

/* Per-sequence camera model (ABI 11), camodocal's CameraFactory model_type.  p[] holds, in this order:
 *   VIO_CAMERA_PINHOLE         fx fy cx cy k1 k2 p1 p2       (the pinhole fields of vio_calibration)
 *   VIO_CAMERA_KANNALA_BRANDT  k2 k3 k4 k5 mu mv u0 v0       (EquidistantCamera)
 *   VIO_CAMERA_MEI             xi k1 k2 p1 p2 gamma1 gamma2 u0 v0   (CataCamera)
 * and zeros after them.  reserved must be 0.  The back-end is model-free: it works on normalised-plane points (x / z, y / z). */
enum { VIO_CAMERA_PINHOLE = 0, VIO_CAMERA_KANNALA_BRANDT = 1, VIO_CAMERA_MEI = 2 };
typedef struct vio_camera {
    int32_t model, reserved;
    double p[12];
} vio_camera;

/* parameters.cpp:81-243 readParameters() defaults for config/realsense/vio.yaml at 150 features */
void vio_config_default(vio_config *cfg);

/* Estimator::Estimator + setParameter() (estimator.cpp:9-41) for S sequences on the current HIP device.
 * imu_capacity = ring size per sequence (samples). Returns NULL on failure (see vio_last_error): no HIP device (there is no CPU
 * fallback), an allocation that failed, or a configuration whose kernels would need more LDS than a workgroup may own (window size /
 * landmark capacity / feature count beyond what a CU's 160 KB hold) -- checked here so that it cannot surface as a failed launch
 * in the middle of a frame. */
vio_batch *vio_create(const vio_config *cfg, int n_seq, int imu_capacity);
/* The same on a named HIP device (device < 0: the calling thread's current device, i.e. vio_create).  The handle OWNS its device: all of its
 * memory, streams and events live there, and every entry point that takes the handle makes that device current for the duration of the call
 * and restores the caller's afterwards -- so one process may drive one handle per GPU from one thread or from a thread per GPU
 * without ever calling hipSetDevice itself.  Device pointers passed with on_device != 0 must belong to the handle's device.  No upstream
 * counterpart (the reference is one Estimator per process on the CPU). */
vio_batch *vio_create_on_device(const vio_config *cfg, int n_seq, int imu_capacity, int device);
int vio_get_device(vio_batch *h);   /* the device the handle lives on; VIO_EINVAL for NULL */
void vio_destroy(vio_batch *h);
const char *vio_last_error(void);
/* Every sequence back to the state after vio_create: fresh FeatureTracker AND Estimator::clearState() + setParameter(). */
int vio_reset(vio_batch *h);

/* Estimator::inputIMU(t, acc, gyr) (estimator.cpp:1749-1766) for sequence seq; n samples, t strictly increasing. */
int vio_push_imu(vio_batch *h, int seq, int n, const double *t, const double *acc_xyz, const double *gyr_xyz);
/* The same for every sequence in one call (SURVEY.md 8b "batched variants taking SoA pointers"): n[s] samples for sequence s,
 * stored at t[s * stride + i], acc_xyz / gyr_xyz[(s * stride + i) * 3 + k]; n == NULL means `stride` samples for every sequence. */
int vio_push_imu_batch(vio_batch *h, const int32_t *n, int stride, const double *t, const double *acc_xyz, const double *gyr_xyz);
/* Estimator::clearState() + setParameter() for ONE sequence (estimator.cpp:15-116): what the stream-discontinuity branch of
 * process_tracker does (estimator_nodelet.cpp:243-262) -- window, landmarks, prior, pre-integrations and the buffered IMU of that
 * sequence are dropped, the pending feature map is discarded (feature_buf popped, :250-253), the nodelet's first_image_flag is set
 * again and last_image_time zeroed (:246-247; they only matter to vio_feed's device-side gating).  The FeatureTracker is NOT touched:
 * trackerData keeps its points, ids, track counts and previous image, init_pub / init_feature keep their values, exactly as upstream. */
int vio_reset_seq(vio_batch *h, int seq);
/* A fresh FeatureTracker for one sequence (no upstream counterpart: the reference only ever constructs its tracker once). */
int vio_reset_tracker_seq(vio_batch *h, int seq);

/* One camera frame for every sequence: the body of EstimatorNodelet::process_tracker for one synchronised
 * colour+depth pair (estimator_nodelet.cpp:234-393) followed by EstimatorNodelet::process (:462-549):
 *   predictMotion (estimator.cpp:1790-1860) -> FeatureTracker::readImage (feature_tracker.cpp:263-439) -> updateID loop
 *   -> feature-map packaging -> FeatureManager::inputDepth -> Estimator::processImage (estimator.cpp:156-374).
 * gray: S images [S][height][width] u8, depth_mm: [S][height][width] u16 (CV_16UC1 millimetres).
 * on_device != 0: pointers are HBM addresses (no PCIe in the call); otherwise host buffers that are uploaded first.
 * stamps: S timestamps (seconds). The call is asynchronous on the batch's stream; vio_sync or any getter waits.
 * Per-sequence status codes are read back with vio_get_status. */
/* Host IMAGE buffers (on_device == 0) are uploaded by a copy stream beside the previous frames' kernels, two uploads in flight: pageable
 * buffers are free when the call returns (the runtime stages them), page-locked ones (vio_host_alloc) when vio_host_buffers_done says so and at
 * the latest once the SECOND next vio_feed / vio_feed_modes call on the handle (or any getter / vio_sync) has returned.  `stamps` (and `modes`)
 * are copied into a library-owned page-locked ring before the call returns: they are free at once, page-locked or not. */
int vio_feed(vio_batch *h, const uint8_t *gray, const uint16_t *depth_mm, const double *stamps, int on_device);
/* Non-blocking: 1 if the image uploads of the vio_feed call issued `calls_ago` calls ago (0 = the latest) have completed and its host buffers
 * may be rewritten, 0 if they are still in flight; calls_ago >= 2 is always 1.  No upstream counterpart (the reference's images arrive as ROS
 * messages it owns). */
int vio_host_buffers_done(vio_batch *h, int calls_ago);

/* The two halves of vio_feed, exposed separately the way the reference exposes them to its two threads.
 * vio_track   = predictMotion + readImage(img, t, relative_R) + updateID + packaging; publish = PUB_THIS_FRAME.
 * vio_process = inputDepth + processImage on the features packaged by the last vio_track. */
int vio_track(vio_batch *h, const uint8_t *gray, const double *stamps, int publish, int on_device);
int vio_process(vio_batch *h, const uint16_t *depth_mm, int on_device);
int vio_sync(vio_batch *h);

/* Per-sequence frame modes = the outcome of the nodelet's frequency control for one frame (estimator_nodelet.cpp:264-286):
 * SKIP    the frame is dropped before readImage ("Skip this frame", :266-271): no state changes at all;
 * TRACK   readImage with PUB_THIS_FRAME == false: LK + culling + track_cnt++ only, no RANSAC / mask / detection
 *         (feature_tracker.cpp:351), nothing handed to processImage;
 * PUBLISH readImage with PUB_THIS_FRAME == true + processImage. */
enum { VIO_FRAME_SKIP = 0, VIO_FRAME_TRACK = 1, VIO_FRAME_PUBLISH = 2 };
/* vio_feed with a mode per sequence (modes[S], host memory; NULL = PUBLISH for all). */
int vio_feed_modes(vio_batch *h, const uint8_t *gray, const uint16_t *depth_mm, const double *stamps, const uint8_t *modes, int on_device);
/* vio_track with a mode per sequence and an optional caller-supplied relative rotation per sequence:
 * FeatureTracker::readImage(img, cur_time, relative_R) (feature_tracker.h:36-37).  R_rel: [S][9] row-major host memory or NULL;
 * a NaN in the first element of a sequence's matrix = predict it on the device (Estimator::predictMotion). */
int vio_track_ex(vio_batch *h, const uint8_t *gray, const double *stamps, const uint8_t *modes, const double *R_rel, int on_device);
/* Estimator::predictMotion(t0, t1) (estimator.cpp:1790-1860) for sequence seq on the IMU pushed so far: R[9] row-major. */
int vio_predict_motion(vio_batch *h, int seq, double t0, double t1, double *R9);
/* Estimator::processImage(image, header) (estimator.h:46, estimator.cpp:156-374) + FeatureManager::inputDepth with a CALLER-SUPPLIED
 * feature map for sequence seq: n entries in ascending feature id (std::map order), xyz_uv_vel[n][7] = (x, y, z = 1, u, v, vx, vy)
 * exactly as estimator_nodelet.cpp:336-363 packs them, depth_mm = the CV_16UC1 depth image of THAT frame (host memory), stamp =
 * header stamp.  This is what the process thread pops from feature_buf (estimator_nodelet.cpp:380-384, 539), so the tracker may
 * run ahead of the estimator by any number of frames.  n <= the tracker capacity (max_cnt + grid slack, see vio_get_capacity).
 * Feature ids are NON-NEGATIVE, as the reference's are (its tracker counts them up from 0): -1 is the empty key of the back end's
 * id -> slot table.  A map with a negative id is refused with VIO_EINVAL (text in vio_last_error) before anything is uploaded or
 * launched; the sequence is untouched.  The order of the entries is free: the landmarks a map introduces are appended in the map's order
 * (ascending ids reproduce the reference's list order).
 * IMU: the samples of one frame interval are kept per window slot (64 of them) for as long as the sequence runs, because a non-keyframe's
 * samples are re-propagated into the previous slot (MARGIN_SECOND_NEW).  A frame interval with more than 64 samples, i.e. an IMU rate above
 * 64 x the rate of processed frames, raises overflow flag 2 and that merge then misses the samples beyond the 64th. */
int vio_process_obs(vio_batch *h, int seq, int n, const int32_t *ids, const double *xyz_uv_vel, const uint16_t *depth_mm, double stamp);
/* The same for the whole batch: n_obs[S] (a negative count skips the sequence), ids[S][cap], xyz_uv_vel[S][cap][7], depth_mm
 * [S][height][width], stamps[S]; the feature arrays are host memory, depth_mm is HBM when on_device != 0.  A negative id in any sequence's
 * map refuses the whole call with VIO_EINVAL, as above.  (The maps that reach the back end from device memory -- vio_process, vio_feed: what
 * the handle's own tracker packaged -- cannot be checked by the host; their ids are non-negative by construction, and a caller that writes
 * such device buffers itself must keep that precondition.) */
int vio_process_obs_batch(vio_batch *h, const int32_t *n_obs, const int32_t *ids, const double *xyz_uv_vel, int cap,
                          const uint16_t *depth_mm, const double *stamps, int on_device);
/* The feature map packaged by the last vio_track / vio_feed for sequence seq (what the nodelet would push to feature_buf):
 * returns the count (0 when the frame was not published), ids ascending. */
int vio_get_packaged(vio_batch *h, int seq, int cap, int32_t *ids, double *xyz_uv_vel);
/* HBM buffers for callers that do not link HIP themselves (the on_device != 0 arguments are plain device addresses): synchronous
 * hipMalloc / hipFree / hipMemcpy on the current device.  vio_device_alloc returns NULL on failure. */
void *vio_device_alloc(size_t bytes);
void vio_device_free(void *p);
int vio_device_upload(void *dst_device, const void *src_host, size_t bytes);
int vio_device_download(void *dst_host, const void *src_device, size_t bytes);
/* page-locked host memory for the on_device == 0 image arguments: uploads from it run at PCIe rate and asynchronously (from pageable
 * memory the runtime stages every copy).  NULL on failure. */
void *vio_host_alloc(size_t bytes);
void vio_host_free(void *p);
/* sizeof(vio_config) (what = 0) / sizeof(vio_status) (what = 1) / sizeof(vio_calibration) (what = 2) / sizeof(vio_camera) (what = 3) /
 * sizeof(vio_snapshot_header) (what = 4) / sizeof(vio_snapshot_shape) (what = 5) as compiled into the library: lets a binding check its
 * struct mirrors */
int vio_abi_sizeof(int what);
/* Contract version of this header: 4 = a vio_feed host image set is free when the next vio_feed has returned; 5 = two uploads in flight (see
 * "Host buffers" above, vio_host_buffers_done); 6 = + vio_get_bound_stats, the inverse-depth bound handled as Ceres does (projected line search);
 * 7 = + estimate_extrinsic = 2 (vio_get_ex_calibration, vio_stage_relative_r); 8 = overflow flag 128 means only "extrinsic-calibration history
 * full": the fallback solver's clamp-only treatment of a bounded landmark moved to flag 512 (VIO_OVF_DEVIATION), which is no capacity error,
 * and flag 256 is documented (vio_status); 9 = + stage harnesses of the remaining be_linalg.h primitives (vio_stage_jacobi, vio_stage_sym_eig_lds,
 * vio_stage_spd_inverse16, vio_stage_scan_flags, vio_stage_schur, vio_stage_pinv15, vio_stage_chol blocks = -8 / -9); 10 = + per-sequence
 * calibration (vio_calibration, vio_calibration_from_config, vio_set_calibration, vio_get_calibration, vio_abi_sizeof(2)); 11 = + per-sequence
 * camera models (vio_camera, vio_set_camera, vio_get_camera, vio_stage_camera, vio_stage_host_camera, vio_abi_sizeof(3);
 * vio_synth_render_host_camera / _device_camera in vio_synth.h, vio_pg_describe_camera in vio_posegraph.h); 12 = + sequence snapshots
 * (vio_snapshot_header, vio_shape_key, vio_snapshot_bytes, vio_save_seqs, vio_load_seqs, vio_snapshot_info, vio_abi_sizeof(4) / (5)). */
int vio_abi_version(void);
/* capacities derived from the configuration: out[0] = tracker points per sequence, out[1] = landmark slots, out[2] = IMU ring */
int vio_get_capacity(vio_batch *h, int32_t *out3);
/* which solver the handle's configuration selected: 0 = the persistent one-workgroup-per-sequence kernel (fallback), 1 = the phased solver
 * with the Schur complement resident in LDS (windows up to W = 10), 2 = the phased solver with it in HBM / L2 (larger windows) */
int vio_get_solver_kind(vio_batch *h);
/* Bounds-constrained solves (estimator.cpp:1282-1297: SetParameterUpperBound(para_Feature, 0, 2 / DEPTH_MAX_DIST) on landmarks triangulated
 * without a depth measurement, which makes Ceres project x0 onto the box and run its Armijo line search along every step).  Counters of
 * sequence seq since vio_create / vio_reset: out4 = {inverse depths cut by the bound while a point was formed, bounded landmarks that
 * entered solves, trial evaluations of the line search, shortened steps}; the fallback solver (vio_get_solver_kind() == 0) counts the first
 * two and runs no line search.  Synchronises the device. */
int vio_get_bound_stats(vio_batch *h, int seq, int64_t *out4);
/* vio_config.marg_exact = 2 only: out2 = {marginalisations of sequence seq whose certificate FAILED since vio_create / vio_reset (such a frame
 * keeps the block inverse without the proof that the reference's 1e-8 eigenvalue cut of marginalization_factor.cpp:281-291 drops nothing),
 * 1 if the last marginalisation was certified}.  Synchronises the device. */
int vio_get_marg_certificate(vio_batch *h, int seq, int32_t *out2);
/* estimate_extrinsic = 2: InitialEXRotation of sequence seq (initial_ex_rotation.cpp:12-68).  Every processed frame with frame_count != 0 of a
 * calibrating sequence appends one pair (Rc = solveRelativeR of the correspondences of window frames frame_count - 1 and frame_count, Rimu = the
 * delta_q of that frame's pre-integration, Rc_g = ric^-1 Rimu ric with the estimate of ric at that time) and re-solves the Huber-weighted
 * averaging; success (calls >= window_size and the third singular value > 0.25) sets the sequence's ric, after which the initialisation runs and
 * the solver refines ric / tic as in mode 1.  out16 = {state: 2 calibrating, 1 calibrated, 0 the handle is not in mode 2; stored pairs;
 * frames_processed (vio_status) after the frame that succeeded, -1 while calibrating; the current estimate of ric (9, row-major); the four
 * singular values of the last averaging step, descending}.  history (may be NULL when cap = 0) receives the oldest min(cap, pairs) stored pairs
 * as 12 doubles each: q(Rc), q(Rimu), q(Rc_g) (w x y z, Eigen's matrix -> quaternion rule).  At most 2048 pairs are kept per sequence (the
 * reference's list is unbounded): beyond that the oldest is dropped and the frame raises overflow flag 128.  vio_reset starts the calibration
 * over; vio_reset_seq and a failure-detection reboot keep a calibrated rotation (with tic = 0), as setParameter() restores RIC[0] upstream.
 * Returns the number of stored pairs (0 for a handle not in mode 2).  Synchronises the device. */
int vio_get_ex_calibration(vio_batch *h, int seq, double *out16, int cap, double *history);

/* Results read out of the path (SURVEY.md §8b "Results read out").  All getters synchronise first. */
enum { VIO_OVF_DEVIATION = 512 };   /* vio_status.overflow_flags bit that reports a deviation, not lost capacity */
typedef struct vio_status {
    int32_t code;                 /* VIO_OK / VIO_NEED_IMU / VIO_REBOOTED of the last vio_process */
    int32_t solver_flag;          /* 0 INITIAL, 1 NON_LINEAR (estimator.h SolverFlag) */
    int32_t frame_count;
    int32_t marginalization_flag; /* 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW */
    int32_t n_landmarks;          /* f_manager.feature.size() */
    int32_t last_track_num;
    int32_t n_tracks;             /* FeatureTracker::ids.size() */
    int32_t processed;            /* 1 if processImage ran for the last frame */
    int32_t iterations, successful_steps;
    int32_t n_in_problem, n_residuals, n_var_landmarks, has_prior;
    int32_t reboot_count, frames_processed;
    double initial_cost, final_cost, td;
    int32_t overflow_flags;       /* capacity flags of the last frame: 1 landmark table, 2 IMU slot (> 64 samples per frame interval: IMU rate / frame rate must be <= 64, see vio_process_obs),
                                     4 FAST candidates of a cell, 8 residual list, 16 IMU ring overwritten, 32 solver iteration slots
                                     exhausted before the trust-region loop finished, 64 relocalisation request dropped (vio_set_relo_frame),
                                     128 extrinsic-calibration history full: its oldest pair was dropped (estimate_extrinsic = 2, see
                                     vio_get_ex_calibration), 256 a solve skipped: it did not fit the fused evaluate + assemble kernel on a
                                     handle that launches nothing else (VIO_FUSE), the window is left unoptimised (code = VIO_ECAPACITY
                                     for any of these); 512 (VIO_OVF_DEVIATION) NOT a capacity flag: the fallback solver
                                     (vio_get_solver_kind() == 0) met a landmark under the inverse-depth bound and clamped its candidates
                                     instead of running Ceres' projected line search -- a deviation from the reference; it leaves code and
                                     overflow_frames alone */
    int32_t overflow_frames;      /* frames that raised any capacity flag (512 excepted) since the last reset / reboot */
    int32_t iterations_total, solves_total; /* solver iterations / solves since vio_create */
} vio_status;
int vio_get_status(vio_batch *h, int seq, vio_status *out);
/* the same for every sequence of the handle in two device reads: out[n_seq] */
int vio_get_status_all(vio_batch *h, vio_status *out);
/* window state Ps/Rs/Vs/Bas/Bgs/Headers (estimator.h:121-135): (W+1) rows of 17 doubles
 * [P(3) Q(w,x,y,z) V(3) Ba(3) Bg(3) stamp] */
int vio_get_window(vio_batch *h, int seq, double *out);
/* the CSV row of visualization.cpp:214-225 for every sequence: [S][11] = stamp, P(3), Q(w,x,y,z), V(3) of frame W */
int vio_get_odometry(vio_batch *h, double *out);
/* CSV rows written for sequence seq.  The device keeps a ring of the last 2048 rows: out receives the most recent min(rows, 2048,
 * cap) of them in time order; returns the number of rows produced since vio_create / the last reset (may exceed what fits). */
int vio_get_odometry_history(vio_batch *h, int seq, int cap, double *out);
/* FISHEYE (parameters.cpp:111-114, estimator.cpp:29-36): FeatureTracker::setMask starts from fisheye_mask instead of an all-255 image
 * (feature_tracker.cpp:175-176), so tracked and new features are only kept where the mask is 255 and FAST corners only where it is not 0.
 * mask = ROW x COL u8 (the decoded config/fisheye_mask.jpg; decoding is the caller's), shared by all sequences of the handle; NULL turns
 * the option off.  Synchronises the handle. */
int vio_set_fisheye_mask(vio_batch *h, const uint8_t *mask, int on_device);
/* How far the estimator runs behind the tracker inside vio_feed / vio_feed_modes.  The reference's process_tracker and process()
 * threads run concurrently (estimator_nodelet.cpp:192-459 / :462-549): Estimator::predictMotion of frame f+1 reads latest_Bg / td as the
 * estimator thread left them, i.e. after frame f when the estimator keeps up and after frame f-1 when it is still optimising frame f.
 *   lag 0 (default): the tracker of frame f+1 starts after the optimisation of frame f (estimator keeps up);
 *   lag 1: it reads the state as of frame f-1 (a snapshot be_ingest takes) and overlaps the optimisation of frame f, which takes
 *          the front-end off the critical path.  Results are deterministic in both modes; the oracle implements the same two
 *          orderings (ovio_set_tracker_lag).  Not available on dynamic_init handles.  vio_track / vio_process_obs callers choose the
 *          ordering themselves.
 * Changing the lag synchronises the handle and re-creates its streams (with lag 1 the front-end streams are confined to their own
 * compute units): a stream obtained from vio_get_stream before the call is no longer valid. */
int vio_set_tracker_lag(vio_batch *h, int lag);
/* the IMU-rate pose of pubLatestOdometry (Estimator::predict, estimator.cpp:1862-1880, fed by inputIMU :1749-1766 after
 * updateLatestStates :1768-1788): the newest window state propagated through every IMU sample pushed after it.
 * out11 = t, P(3), Q(w, x, y, z), V(3).  INITIAL sequences and VO mode return the window state unchanged. */
int vio_get_latest_odometry(vio_batch *h, int seq, double *out11);
/* vio_get_latest_odometry for every sequence in one launch and one copy: out[S][11], the same bits per row.  on_device != 0: out is an
 * HBM address on the handle's device and nothing but the launch crosses the bus. */
int vio_get_latest_odometry_all(vio_batch *h, double *out, int on_device);
/* The IMU-rate stream itself: pubLatestOdometry publishes one pose per IMU sample, and this returns, for every sequence, the row
 * t, P(3), Q(w, x, y, z), V(3) after EVERY sample newer than the window state (row k is what vio_get_latest_odometry returned when the
 * k-th of them had just been pushed, bit for bit).  One launch and one copy for the whole batch.
 *   since   [S] host doubles or NULL: only rows with t > since[s] are counted and returned, so a poller passes the last stamp it has
 *           received and gets the new rows only.  The propagation still starts at the window state: an optimisation in between
 *           re-anchors the rows, as it does upstream.  NULL: every applied sample.
 *   n_rows  [S] host: the number of such rows, which may exceed cap
 *   out     [S][cap][11]: the first min(n_rows[s], cap) rows of sequence s in time order; rows beyond them are left untouched.
 *           on_device != 0: an HBM address on the handle's device (only n_rows comes back to the host).  cap == 0 (out may be NULL) only counts.
 * The bytes copied back grow with S * cap, whatever n_rows turns out to be: a poller sets cap near the rows it expects per poll.
 * INITIAL sequences and VO mode apply no sample: n_rows[s] = 0.  Samples the ring has overwritten (imu_capacity) are not applied. */
int vio_get_imu_rate_odometry(vio_batch *h, const double *since, int cap, int32_t *n_rows, double *out, int on_device);
/* pubPointCloud (visualization.cpp:328-407) and pubKeyframe (visualization.cpp:454-520) for every sequence: one launch and one copy for
 * the whole batch, where vio_get_landmarks_ex + vio_get_window + vio_get_extrinsic take about a dozen copies per sequence.  Every list is
 * in the order of f_manager.feature (the order of vio_get_landmarks).
 *   counts     [S][4] host: n_cloud, n_margin, n_kf, kf_valid.  The full numbers, which may exceed cap.  kf_valid = 1 where the sequence is
 *              NON_LINEAR, the last frame was processed and its marginalization_flag is MARGIN_OLD: the frames for which pubKeyframe
 *              publishes.  n_kf = 0 otherwise.
 *   kf_pose    [S][8]: Headers[W-2], Ps[W-2], Q(w, x, y, z) of Rs[W-2], the bits of row W-2 of vio_get_window.  Rows of sequences with
 *              kf_valid = 0 are left untouched.
 *   cloud      [S][cap][3]: the world point of every landmark pubPointCloud keeps (not dynamic, n_obs >= 2, start_frame < W-2, not
 *              start_frame > 3W/4, solve_flag 1)
 *   margin     [S][cap][3]: pubPointCloud's margin cloud (the same first tests, then start_frame 0, n_obs <= 2, solve_flag 1)
 *   kf_points  [S][cap][8]: per landmark that spans window frame W-2 with start_frame < W-2 and solve_flag 1, dynamic or not: the world
 *              point, then x, y, u, v of its observation in frame W-2 and its feature id
 * Rows beyond min(count, cap) are left untouched.  Any of cloud, margin, kf_points may be NULL: that list is only counted; cap == 0 counts
 * everything.  on_device != 0: kf_pose and the three lists are HBM addresses on the handle's device and only counts comes back to the host.
 * The bytes copied back grow with S * cap whatever the counts turn out to be.  Reads only; waits for all work of the handle. */
#define VIO_PUBLISH_BLOCK 256   /* landmarks per step of the list walk (the workgroup size of the launch) */
int vio_publish_all(vio_batch *h, int cap, int32_t *counts, double *kf_pose, double *cloud, double *margin, double *kf_points, int on_device);
/* Estimator::setReloFrame(frame_stamp, frame_index, match_points, relo_t, relo_r) (estimator.h:48-49, estimator.cpp:1728-1747) for
 * sequence seq: the window frame stamped frame_stamp has been matched with an old keyframe (pose relo_t / relo_r in the loop-closed
 * world, relo_r row-major); match_points[n][3] = (x, y) normalised point of the old keyframe and the feature id it matched (z), in
 * ascending id like the pose graph sends them (pose_graph/src/keyframe.cpp).  If the stamp is one of Headers[0 .. W-1] the NEXT
 * optimisation of that sequence carries the relocalisation factors (estimator.cpp:1307-1346: ProjectionFactor(first observation,
 * matched point) on (para_Pose[start], relo_Pose, extrinsic, inverse depth) for every in-problem landmark with start_frame <=
 * relo_frame_local_index among the matches) and computes the drift outputs (:1034-1056); otherwise nothing happens, like upstream.
 * relo_Pose borrows the six tangent columns of the extrinsic in the reduced system: when ESTIMATE_EXTRINSIC has opened the extrinsic it is
 * held constant in the ONE solve that carries the factors and refined again from the next solve on (DESIGN.md deviation 15: below a
 * millimetre against the joint optimisation).  Limits of this build: IMU mode and the phased solver.  On the persistent solver (windows
 * beyond its range, VIO_SOLVE_MODE=0) and on a handle with use_imu = 0 (VO mode) a latched request is dropped by the next solve of the
 * sequence: that frame carries overflow flag 64, vio_get_relo reports pending = 0 and 0 factors, and the frame is otherwise computed as if
 * the request had never been made.  A request made before the first optimisation copies an identity pose (the reference copies from an
 * array it has not written yet); it waits for the solve that ends the initialisation, which carries its factors. */
int vio_set_relo_frame(vio_batch *h, int seq, double frame_stamp, int frame_index, int n, const double *match_points, const double *relo_t3,
                       const double *relo_r9);
/* what pubRelocalization and the pose graph read after that solve (visualization.cpp:454-538): out30 = relo_relative_t(3),
 * relo_relative_q(w x y z), relo_relative_yaw (degrees), drift_correct_t(3), drift_correct_r(9 row-major), relo_Pose(7: p, q x y z w),
 * relocalization_info (1 = still pending), relo_frame_local_index, number of relocalisation factors of the last solve */
int vio_get_relo(vio_batch *h, int seq, double *out30);
/* tic(3), ric(9 row-major), td */
int vio_get_extrinsic(vio_batch *h, int seq, double *out13);
/* The calibration fields of cfg (no validation). */
void vio_calibration_from_config(const vio_config *cfg, vio_calibration *out);
/* Gives sequence seq its own sensor calibration.  A slot with calibration k computes, bit for bit, what slot 0 of a one-sequence handle created
 * with the handle's configuration and k's fields computes.  Validated first: every value finite, fx, fy > 0, tr >= 0, acc_n, acc_w, gyr_n, gyr_w,
 * g_norm > 0, ric a rotation (orthonormal within 1e-6, determinant +1); otherwise VIO_EINVAL with vio_last_error() naming the field, and the
 * slot is left untouched.  ric is re-orthonormalised through a normalised quaternion as vio_create does with cfg->ric; on an
 * estimate_extrinsic = 2 handle ric / tic become I / 0.  On success the slot restarts like a freshly created handle (synchronises as
 * vio_reset_seq, then a fresh tracker and estimator: IMU ring and last IMU stamp, mode-2 calibration history, sticky diagnostics), so the new
 * sensor's clock may start again from 0.  Other slots are not disturbed.  The calibration persists across vio_reset, vio_reset_seq,
 * vio_reset_tracker_seq and the failure-detection reboot (which restores ric / tic / td / g from it; mode 2 keeps its calibrated rotation). */
int vio_set_calibration(vio_batch *h, int seq, const vio_calibration *cal);
/* The calibration in effect for seq: ric after re-orthonormalisation, I / 0 on estimate_extrinsic = 2 handles (vio_get_extrinsic returns the
 * current estimate instead). */
int vio_get_calibration(vio_batch *h, int seq, vio_calibration *out);
/* Gives sequence seq its own camera model (feature_tracker.cpp:500, CameraFactory::generateCameraFromYamlFile).  The tracker lifts and projects
 * through it (predictPtsInNextFrame, rejectWithF, undistortedPoints); everything downstream sees normalised-plane points x / z, y / z.  A slot
 * with camera k computes, bit for bit, what slot 0 of a one-sequence handle given camera k computes.  Validated first: model known, reserved
 * 0, every p[] finite, fx, fy, mu, mv, gamma1, gamma2 > 0, xi >= 0, and the four image corners and four edge midpoints lift to finite rays
 * with z > 0 (the unit-plane factors cannot represent a ray at or beyond 90 degrees); otherwise VIO_EINVAL with vio_last_error() naming the
 * field, and the slot is left untouched.  PINHOLE writes fx..p2 into the slot's vio_calibration.  On success the slot restarts as with
 * vio_set_calibration; other slots are not disturbed.  vio_create gives every slot PINHOLE from cfg; vio_set_calibration never changes the
 * model (its fx..p2 take effect while the model is PINHOLE); the camera persists across vio_reset* and the failure-detection reboot. */
int vio_set_camera(vio_batch *h, int seq, const vio_camera *cam);
/* The camera of seq (PINHOLE: p[] = the calibration's fx..p2). */
int vio_get_camera(vio_batch *h, int seq, vio_camera *out);
/* ---- sequence snapshots (ABI 12): take a running sequence out of a slot and put it into another one ----
 * A snapshot is one self-describing blob in HOST memory (pageable or page-locked) that holds everything the next vio_feed / vio_track /
 * vio_process* of that sequence reads: tracker and estimator records, the W + 2 pre-integrations, both ping-pong images and pyramids, the
 * tracker arrays, the packaged observations, the IMU ring (samples pushed for future frames included), the landmark table, the prior, a
 * pending relocalisation request, the odometry rows, the sticky counters, the mode-2 extrinsic calibration and its pair ring, the slot's
 * vio_calibration and vio_camera, and the host side (the last IMU stamp; on dynamic_init handles the image-frame mirror of a sequence that is
 * still INITIAL, which is the variable-length part).  Per-frame scratch is not saved.  A blob restores into ANY slot of ANY handle whose
 * shape key and tracker lag equal the source's: the batch size, the slot index, the device and the process may all differ, and the restored
 * sequence continues bit for bit like the original.  NOT in a snapshot, the caller's to set equal on both sides: the fisheye mask
 * (handle-wide), the VIO_* environment knobs read at vio_create, profiling state, and caller-side state such as a frame gate.
 *
 * Layout: vio_snapshot_header | device part (the state arrays of the slot in the order of the layout table, DESIGN.md 6d, every entry on a
 * 16-byte boundary) | host part.  All padding is zero: equal states give equal bytes. */
#define VIO_SNAPSHOT_MAGIC 0x0050414E534F4956ULL   /* "VIOSNAP\0", little endian */
#define VIO_SNAPSHOT_FORMAT 1
/* Shape key: every configuration value that sizes an array or selects a code path, i.e. vio_config without the fields of
 * vio_calibration, plus the capacities fixed at vio_create.  Two handles exchange snapshots exactly when their keys are equal. */
typedef struct vio_snapshot_shape {
    int32_t width, height, max_cnt, min_dist, grid_rows, grid_cols, window_size, max_landmarks, fix_depth, estimate_extrinsic, estimate_td,
        max_iterations, ransac_max_iters, lk_max_level, dynamic_init, use_imu, reference_quirks, marg_exact, equalize;
    int32_t imu_capacity;     /* IMU ring size per sequence as vio_create rounds it (>= 256) */
    int32_t hist_cap;         /* odometry rows kept per sequence */
    int32_t pyramid_levels;   /* pyramid levels stored beside level 0 */
    int32_t reserved[2];      /* 0 */
    double focal_length, f_threshold, depth_min, depth_max, min_parallax_px, init_depth;
} vio_snapshot_shape;
typedef struct vio_snapshot_header {
    uint64_t magic;             /* VIO_SNAPSHOT_MAGIC */
    uint32_t format_version;    /* VIO_SNAPSHOT_FORMAT */
    uint32_t abi_version;       /* vio_abi_version() of the library that wrote the blob */
    int64_t total_bytes;        /* the whole blob = sizeof(vio_snapshot_header) + device_bytes + host_bytes */
    int64_t device_bytes;       /* fixed by the shape key */
    int64_t host_bytes;         /* variable (dynamic_init handles), a multiple of 16 */
    int64_t frames_processed;   /* informational: vio_status.frames_processed of the sequence */
    double last_stamp;          /* informational: header stamp of the last processed frame */
    int32_t tracker_lag;        /* vio_set_tracker_lag of the source handle: must equal the destination's */
    int32_t solver_flag;        /* informational: 0 INITIAL, 1 NON_LINEAR */
    vio_snapshot_shape shape;
} vio_snapshot_header;
/* The shape key of a handle created with (cfg, imu_capacity).  Host only (no GPU, no handle).  Independent of the batch size and of every
 * vio_calibration / vio_camera field. */
int vio_shape_key(const vio_config *cfg, int imu_capacity, vio_snapshot_shape *out);
/* Validates and describes a blob without a handle and without a GPU: magic, format version, the lengths against `bytes`; never reads beyond
 * blob + bytes.  VIO_EINVAL (vio_last_error names the field) for NULL, an empty or short buffer, a wrong magic, an unknown format version or
 * inconsistent lengths. */
int vio_snapshot_info(const void *blob, int64_t bytes, vio_snapshot_header *out);
/* Bytes vio_save_seqs would write for seq right now (the fixed device part + the variable host part); < 0 on error.  Synchronises the
 * handle on dynamic_init handles (the host part depends on the last frame's outcome). */
int64_t vio_snapshot_bytes(vio_batch *h, int seq);
/* Saves n sequences: blob i starts at (char *)dst + offsets[i] and may use caps[i] bytes; bytes_out[i] (may be NULL) = bytes written.
 * Save only READS the handle: it moves the IMU samples still staged on the host into the rings, waits for all work of the handle and picks up
 * a pending reboot notice, as vio_reset_seq does, then copies; the handle continues exactly as if save had not been called.  The slices of
 * the slots are gathered by one kernel per stream group into a device staging buffer (allocated at the first save / load of the handle, never
 * at vio_create) and leave in ONE device-to-host copy when the blobs are packed back to back (offsets[i + 1] = offsets[i] + bytes of blob
 * i, offsets multiples of 16), in one copy per blob otherwise.  VIO_EINVAL: bad slot, VIO_ECAPACITY: caps[i] too small (nothing written). */
int vio_save_seqs(vio_batch *h, int n, const int32_t *seqs, void *dst, const int64_t *offsets, const int64_t *caps, int64_t *bytes_out);
/* Restores n blobs (blob i at (const char *)src + offsets[i], bytes[i] long) into the n DISTINCT slots seqs[i].  Everything is validated
 * before anything is written: magic, versions, lengths, the shape key and the tracker lag against the handle, the blob's calibration and camera
 * as vio_set_calibration / vio_set_camera validate theirs; on any mismatch VIO_EINVAL, vio_last_error names the first field that differs,
 * and every slot is untouched.  On success it synchronises like vio_reset_seq, drops the host-staged IMU of those slots, writes the slots
 * (one host-to-device copy under the same packing rule, then one scatter kernel per stream group) and updates the handle's host mirrors.
 * Other slots are not disturbed.  The same blob may be loaded into several slots (a fork). */
int vio_load_seqs(vio_batch *h, int n, const int32_t *seqs, const void *src, const int64_t *offsets, const int64_t *bytes);
/* test / measurement helpers: the blob of seq written the naive way, one hipMemcpy per layout-table entry (same bytes as vio_save_seqs;
 * returns the bytes written or < 0), and what the handle has reserved on the device for snapshots: the staging buffer's bytes plus a
 * non-zero count for the table and the sequence list; 0 until the first save / load of the handle. */
int64_t vio_debug_save_seq_naive(vio_batch *h, int seq, void *dst, int64_t cap);
int64_t vio_debug_snapshot_staging_bytes(vio_batch *h);
/* The layout table: entry i of the table as (name, kind: 1 state / 0 scratch, bytes per sequence, offset inside the device part or -1);
 * returns the number of entries (i out of range: that count, nothing written). */
int vio_debug_snapshot_layout(vio_batch *h, int i, char *name64, int32_t *kind, int64_t *bytes_per_seq, int64_t *blob_offset);
/* test / measurement helper of VIO_PREINT_AHEAD (be_ingest): how often, since vio_create, be_ingest took over a frame's IMU
 * pre-integration computed ahead of it beside the previous frame's marginalisation (out2[0]) and how often it was handed such a result but
 * integrated itself (out2[1]: the sequence was not in steady state, the frame was not processed, or an input had changed), summed over the
 * sequences; per_seq (may be NULL): the same pair for every sequence, [S][2].  All zero on a handle created with VIO_PREINT_AHEAD=0.
 * Waits for all work of the handle. */
int vio_debug_preint_ahead(vio_batch *h, int64_t *out2, int64_t *per_seq);
/* Debug: the marginalisations that ran as two launches (VIO_MARG_SPLIT: be_marg_pre_kernel with the window slide, then be_marg_alg_kernel beside the
 * next frame's be_ingest and ps_setup) since creation, summed over the sequences in *total; per_seq (may be NULL): the count of every sequence, [S].
 * All zero on a handle that keeps the one be_marg launch (VIO_MARG_SPLIT=0, tracker lag 0, marg_exact, VO, dynamic_init, windows whose reduced
 * system does not fit LDS).  Waits for all work of the handle. */
int vio_debug_marg_split(vio_batch *h, int64_t *total, int64_t *per_seq);
/* FeatureTracker public vectors after readImage (estimator_nodelet.cpp:337-343): returns count */
int vio_get_tracks(vio_batch *h, int seq, int cap, int32_t *ids, int32_t *track_cnt, float *cur_pts_xy, float *cur_un_pts_xy,
                   float *pts_velocity_xy);
/* f_manager.feature in list order: 7 doubles per landmark
 * [feature_id, start_frame, n_obs, estimated_depth, estimate_flag, solve_flag, is_dynamic]; returns total count */
int vio_get_landmarks(vio_batch *h, int seq, int cap, double *out);
/* the same plus what pubPointCloud reads (visualization.cpp:333-395): 12 doubles per landmark
 * [feature_id, start_frame, n_obs, estimated_depth, estimate_flag, solve_flag, is_dynamic,
 *  feature_per_frame[0].point (x, y, z), feature_per_frame[0].depth (metres, 0 = none), feature_per_frame.back().depth] */
int vio_get_landmarks_ex(vio_batch *h, int seq, int cap, double *out12);
/* last_marginalization_info in the canonical layout: returns n (0 = none) */
int vio_get_prior(vio_batch *h, int seq, double *J_nxn, double *r_n, double *x0, uint8_t *present);

/* Per-stage device time of the last vio_feed in milliseconds (hipEvent on the batch stream):
 * out[0] front-end, out[1] back-end, out[2] total; plus kernel-level entries, see DESIGN.md. Returns count. */
int vio_get_timings(vio_batch *h, int cap, double *out_ms);
/* Per-kernel HIP-event timing of the next max_steps vio_feed calls, recorded on the batch's streams.
 * vio_profile_end: out_ms[10] = average ms of fe_begin, fe_pyrdown, fe_predict, fe_lk, fe_select, fe_fast, fe_add,
 * be_ingest, be_solve, be_marg (be_finish is fused into be_marg); returns the number of recorded steps (steps driven by
 * vio_track / vio_process instead of vio_feed are not counted). */
int vio_profile_begin(vio_batch *h, int max_steps);
int vio_profile_end(vio_batch *h, int cap, double *out_ms);
/* stream the batch launches on (hipStream_t) so callers can bracket it with their own events */
void *vio_get_stream(vio_batch *h);

/* ---- single stages, exposed for the parity tests (same kernels the pipeline launches) ---- */
/* cv::pyrDown inside calcOpticalFlowPyrLK (feature_tracker.cpp:302-305) */
int vio_stage_pyr_down(const uint8_t *src, int w, int h, uint8_t *dst);
/* cv::createCLAHE(3.0, Size(8, 8))->apply (feature_tracker.cpp:269-275, EQUALIZE) */
int vio_stage_clahe(const uint8_t *src, int w, int h, uint8_t *dst);
/* FastFeatureDetector::detect on a ROI, before the mask filter (feature_tracker.cpp:109-110): returns count, out = x,y,score */
int vio_stage_fast_roi(const uint8_t *img, int W, int H, int rx, int ry, int rw, int rh, int cap, float *out_xys);
/* cv::calcOpticalFlowPyrLK(21x21, maxLevel, {COUNT+EPS,30,0.01}, OPTFLOW_USE_INITIAL_FLOW).  As in OpenCV (buildOpticalFlowPyramid),
   the pyramid stops before the first level that is 21 px or less in width or height: the depth used is
   vio_lk_effective_level(w, h, max_level) = min(max_level, deepest l such that every level 1..l is at least 22 x 22; a level is
   (n + 1) / 2 of the one above).  A call with a larger max_level returns exactly what the call with the effective level returns.
   The batch pipeline applies the same rule to vio_config.lk_max_level (the configuration reads back as it was set). */
int vio_lk_effective_level(int width, int height, int lk_max_level);
int vio_stage_lk(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, int n, const float *prev_pts,
                 float *next_pts_inout, uint8_t *status);
/* cv::findFundamentalMat(FM_RANSAC, F_THRESHOLD, 0.99) on virtual-pinhole points (feature_tracker.cpp:462) */
int vio_stage_ransac(const vio_config *cfg, int n, const float *p1, const float *p2, uint8_t *status);
/* InitialEXRotation::solveRelativeR (initial_ex_rotation.cpp:70-147) through the device code of the calibration phase: corres6[n][6] =
 * (x, y, z) of frame l, (x, y, z) of frame r (normalised points, z = 1); R9 = the rotation it returns, row-major (identity for n < 9) */
int vio_stage_relative_r(int n, const double *corres6, double *R9);
/* The same call, and what it decided on the way: detail8 = model found (0 / 1), RANSAC inlier count, the four triangulation votes of
 * (R1, t) (R1, -t) (R2, t) (R2, -t), which of R1 / R2 was returned (1 / 2, 0 without a model), whether the det(R1) = -1 sign change fired */
int vio_stage_relative_r_detail(int n, const double *corres6, double *R9, int *detail8);
/* IntegrationBase::push_back x n + IMUFactor::Evaluate (integration_base.h:32-162, imu_factor.h:20-205)
 * out: delta_p(3) delta_q(wxyz) delta_v(3) sum_dt jacobian(225) covariance(225); r(15); J = 15x7,15x9,15x7,15x9 */
int vio_stage_imu_factor(const vio_config *cfg, int n, const double *dt, const double *acc, const double *gyr,
                         const double *acc0, const double *gyr0, const double *ba, const double *bg, const double *pose_i,
                         const double *sb_i, const double *pose_j, const double *sb_j, double *preint_out, double *r15,
                         double *J480);
/* ProjectionFactor / ProjectionTdFactor::Evaluate (projection_factor.cpp:22-130, projection_td_factor.cpp:34-150)
 * obs = 9 doubles (x,y,z,u,v,vx,vy,cur_td,depth); J = Ji(2x7) Jj(2x7) Jex(2x7) Jl(2) Jtd(2) */
int vio_stage_projection(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep,
                         double td, const double *obs_i, const double *obs_j, int use_td, double *r2, double *J46);
/* the same factor through the per-residual device routine the marginalisation and the outlier rejection use (the solver's hot loop
 * uses the frame-pair form above) */
int vio_stage_projection_residual(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep,
                                  double td, const double *obs_i, const double *obs_j, int use_td, double *r2, double *J46);
/* cv::solvePnP(SOLVEPNP_ITERATIVE, useExtrinsicGuess) with K = I as FeatureManager::solvePoseByPnP calls it in VO mode
 * (feature_manager.cpp:545-588): obj[n][3], img[n][2] normalised points, rvec3 / tvec3 (Rodrigues vector, translation) in and out */
int vio_stage_pnp(int n, const double *obj, const double *img, double *rvec3, double *tvec3);
/* vio_stage_pnp and the path CvLevMarq took: trace4 = outer iterations, lambda escalations, final lambda exponent (base 10), all six
 * parameters finite (0 / 1).  vio_stage_host_pnp_trace is the host solver of the dynamic initialisation from the same (rvec, tvec) start. */
int vio_stage_pnp_trace(int n, const double *obj, const double *img, double *rvec3, double *tvec3, int *trace4);
int vio_stage_host_pnp_trace(int n, const double *obj, const double *img, double *rvec3, double *tvec3, int *trace4);
/* cv::Rodrigues as the device solvePnP uses it, n items, one thread each.  mode 0: in = r[n][3], out[n][36] = R[9] row-major, then
 * dR/dr_0, dR/dr_1, dR/dr_2 (9 each).  mode 1: in = R[n][9], out = r[n][3].  vio_stage_host_rodrigues: the host copy, no GPU needed. */
int vio_stage_rodrigues(int mode, int n, const double *in, double *out);
int vio_stage_host_rodrigues(int mode, int n, const double *in, double *out);
/* Host-only building blocks of the dynamic (static_init: 0) initialisation (csrc/dyninit_host.cpp), callable without a GPU:
 * cv::solvePnP(ITERATIVE, useExtrinsicGuess) (R9 / t3 in: guess, out: result; returns 1 = converged), cv::solvePnPRansac(EPNP) as
 * solveRelativeRT_PNP uses it (solve_5pts.cpp:248-294), and relativePose + GlobalSFM::construct over a window (estimator.cpp:884-920,
 * initial_sfm.cpp:184-412: tracks as start[nf], nobs[nf], obs = (x, y, depth) per observation; out: reference frame l, q[(W+1)*4]
 * (w x y z), T[(W+1)*3], pts[nf*4] = (solved, X, Y, Z), stats[2] = (BA iterations, points in the BA); returns 0 ok, 1 no frame pair
 * with enough parallax, 2 SfM failed). */
int vio_stage_host_pnp(int n, const double *obj, const double *img, double *R9, double *t3);
/* camera_model.h on n pixels uv[n][2]: ray_out[n][3] = liftProjective (not normalised), un_out[n][2] = (x / z, y / z) as undistortedPoints
 * stores it, uv_out[n][2] = spaceToPlane(R9 * ray) as predictPtsInNextFrame computes it (R9 row-major; NULL = identity).  Any of the outputs
 * may be NULL.  vio_stage_camera runs on the device, vio_stage_host_camera on the CPU (no GPU needed). */
int vio_stage_camera(const vio_camera *cam, int n, const double *uv, const double *R9, double *ray_out, double *un_out, double *uv_out);
int vio_stage_host_camera(const vio_camera *cam, int n, const double *uv, const double *R9, double *ray_out, double *un_out, double *uv_out);
int vio_stage_host_pnp_ransac(int n, const double *obj, const double *img, int max_iters, double thresh, double confidence, double *R9, double *t3);
/* LinearAlignmentWithDepth + RefineGravityWithDepth (initial_aligment.cpp:170-244, 337-405): frames19 = n x {R[9] row-major, T[3], sum_dt,
 * delta_p[3], delta_v[3]}; g_out3 = gravity in the SfM frame, x_out[3 n + 3] = body velocities per frame + the last correction;
 * returns 1 when |g| came out within 1 m/s^2 of g_norm before the refinement. */
int vio_stage_host_alignment(int n, const double *frames19, const double *tic3, double g_norm, double *g_out3, double *x_out);
int vio_stage_host_sfm_window(int window_size, int nf, const int32_t *start, const int32_t *nobs, const double *obs, int32_t *l_out, double *q_out,
                              double *T_out, double *pts_out, double *stats_out);
/* IMUFactor::Evaluate as the solver consumes it: G961 = [J r]^T [J r] (31 x 31 row-major; columns pose_i(6) speedbias_i(9) pose_j(6)
 * speedbias_j(9) | residual) through the wavefront code of the solve kernel (split raw Jacobians, on-the-fly whitening, FP64 MFMA) */
int vio_stage_imu_block(const vio_config *cfg, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                        const double *gyr0, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                        const double *pose_j, const double *sb_j, double *G961);
/* Harnesses of the factor code alone (be_factors.h and the propagation routines of be_preint.h), for tests against the definitions.
 * vio_stage_preint: IntegrationBase(acc0, gyr0, ba, bg) followed by n x propagate (integration_base.h:56-162) through mode 0 = preint_propagate step
 * by step, 1 = preint_propagate_many(append = false), 2 = preint_propagate_many(append = true), the merge of MARGIN_SECOND_NEW, which also files
 * the samples (push_back).  dt[n], acc[n][3], gyr[n][3]; the noise densities are cfg's.  out686 = delta_p(3) delta_q(wxyz) delta_v(3) sum_dt
 * jacobian(225) covariance(225), as vio_stage_imu_factor's preint_out, then the whitening matrix M = chol(cov)^-1 (225, row-major lower triangular,
 * all zero when the covariance has no Cholesky factor).  n_buf_out (may be NULL) = samples filed: min(n, 64) in mode 2, 0 otherwise; buf_out (may be
 * NULL; 64 x 7 doubles) = the sample buffer, (dt, acc[3], gyr[3]) per slot, zero where nothing was filed. */
int vio_stage_preint(const vio_config *cfg, int mode, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                     const double *gyr0, const double *ba, const double *bg, double *out686, int *n_buf_out, double *buf_out);
/* vio_stage_preint_ring: beside modes 0 - 2, what the per-frame integration of be_ingest adds to preint_propagate_many(append = true): the samples
 * come from a ring of `cap` entries (t[cap] stamps, acc[cap][3], gyr[cap][3]; sample q of the n >= 1 lies at index (head + q) % cap) with dt formed
 * on the device -- t[first] - prev_time, stamp differences, cur_time - t[last but one] for the last of n >= 2 -- and Estimator::processIMU's
 * world-state step (estimator.cpp:142-152) runs beside the delta-state recursion.  world31, in: acc_0(3) gyr_0(3) Ps(3) Vs(3) Rs(9 row-major)
 * Bas(3) Bgs(3) g(3); out: acc_0, gyr_0, Ps, Vs, Rs after the n samples, and [30] = be_ingest's overflow bits (2 when more samples than a
 * slot's buffer holds were filed).  The other arguments as vio_stage_preint's. */
int vio_stage_preint_ring(const vio_config *cfg, int n, int head, int cap, const double *t, const double *acc, const double *gyr, double prev_time,
                          double cur_time, double *world31, const double *acc0, const double *gyr0, const double *ba, const double *bg,
                          double *out686, int *n_buf_out, double *buf_out);
/* IntegrationBase::evaluate (integration_base.h:164-195) and the Jacobian blocks of IMUFactor::Evaluate (imu_factor.h:92-201) BEFORE the
 * multiplication by sqrt_info, on a caller-supplied pre-integration: pre461 as above (the covariance is not read), ba / bg = its linearisation
 * biases, gravity (0, 0, cfg->g_norm).  r15 = raw residual; J450 = imu_raw_jacobian, 15 x 30 row-major in tangent coordinates, columns pose_i(6)
 * speedbias_i(9) pose_j(6) speedbias_j(9); Jp465 (in and out) = a 15 x 31 row-major buffer into which four lanes write the four
 * imu_raw_jacobian_part column groups as the solver does: columns 0 .. 29 are overwritten, column 30 (the residual's) is returned as passed in. */
int vio_stage_imu_raw(const vio_config *cfg, const double *pre461, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                      const double *pose_j, const double *sb_j, double *r15, double *J450, double *Jp465);
/* eval_projection_pair, the frame-pair form of ProjectionFactor / ProjectionTdFactor::Evaluate, as the solver calls it: cauchy != 0 multiplies the
 * Jacobian rows by the CauchyLoss(1) weight sqrt(1 / (1 + |r|^2)) and stores it in *wgt (r2 stays unweighted; without cauchy *wgt is returned as
 * passed in); rs = 20: rows [pose_i(6) pose_j(6) ex(6) td inv_depth], of which ext = 0 writes only columns 0 .. 12 (inverse depth at 12); rs = 14
 * (ext must be 0): compact rows [pose_i(6) pose_j(6) inv_depth -].  J (in and out, nJ doubles, 2 rs <= nJ <= 4096): the two rows are written at J[0] and
 * J[rs]; every element the routine does not own -- slot 13 of a compact row, everything from 2 rs on -- is returned as passed in.  The readout
 * time is cfg->tr.  VIO_EINVAL for any other (rs, ext) and for an nJ outside that range; nothing is written then. */
int vio_stage_projection_pair(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep, double td,
                              const double *obs_i, const double *obs_j, int use_td, int cauchy, int rs, int ext, double *r2, double *wgt,
                              double *J, int nJ);
/* PoseLocalParameterization::Plus (pose_local_parameterization.cpp:3-20) and the pose delta of MarginalizationFactor::Evaluate
 * (marginalization_factor.cpp:374-393), one thread per input: plus7[i] = Plus(x7[i], d6[i]); dx6[i] = (x - x0, 2 vec(q0^-1 q), negated unless
 * the scalar part of q0^-1 q is >= 0) for x = x7[i], x0 = x07[i].  Poses are (x y z qx qy qz qw). */
int vio_stage_pose_ops(int n, const double *x7, const double *d6, const double *x07, double *plus7, double *dx6);
/* The device routine behind vio_publish_all on the tables of one synthetic sequence.  tables: lm_order, lm_id, lm_start, lm_nobs, lm_solve_flag,
 * lm_dyn ([NL] int32 each, lm_order = the live slots in list order), lm_depth [NL], lm_obs [NL][W+1][9] (x y z u v vx vy cur_td depth, the row of
 * window frame f at (f + ring_base) % (W+1)), Ps [W+1][3], Rs [W+1][9] row-major, Headers [W+1], ric [9], tic [3]; flags3 = solver_flag,
 * marginalization_flag, processed.  counts4, kf_pose8, cloud [cap][3], margin [cap][3], kf_points [cap][8] are in and out: they travel to the
 * device as passed in and come back whole, so what the kernel did not write is what the caller put there.  Lists may be NULL as above. */
typedef struct vio_publish_tables {
    const int32_t *lm_order, *lm_id, *lm_start, *lm_nobs, *lm_solve_flag, *lm_dyn;
    const double *lm_depth, *lm_obs, *Ps, *Rs, *Headers, *ric, *tic;
} vio_publish_tables;
int vio_stage_publish(int NL, int W, int n_lm, int ring_base, const vio_publish_tables *tables, const int32_t *flags3, int cap, int32_t *counts4,
                      double *kf_pose8, double *cloud, double *margin, double *kf_points);
/* The dense solve at the bottom of every trust-region step (Ceres DENSE_SCHUR on the reduced camera system, estimator.cpp:1251-1263;
 * Eigen LLT underneath) through the LDS-tile Cholesky of the solve kernels: S [16 nb][16 nb] row-major symmetric positive definite
 * (nb <= 11; 12 <= nb <= 24 or blocks = -7: the streaming factorisation of windows beyond 10 keyframes, tiles in HBM -- usec5 is then
 * {factorisation, backward substitution, update of the block columns incl. the wait for their diagonal tiles, panels + tile stores, 0}),
 * rhs [16 nb].  L_out: the lower triangle of the factor (row-major; entries above the diagonal are left as passed in),
 * x_out = S^-1 rhs (NaN when a pivot was not positive), usec5 = {factorisation with the forward substitution riding along, backward
 * substitution, then the factorisation as thread 0 sees it: panels, diagonal block + trailing update, barrier wait}: microseconds inside the kernel, mean over `reps` repetitions, with `blocks` identical workgroups side by side.  blocks = -1 .. -6
 * select the timing micro-modes of tools/chol_bench.py (one diagonal tile, panel tiles, dependent FP64 chains, v_mfma_f64_16x16x4 issue
 * rates; usec5 then carries clock64 ticks / 100 in slots 1 .. 4, L_out / x_out are not written): measurement only, see stage_linalg.hip.  blocks = -8 / -9:
 * the HBM fallback of be_solve instead (chol_blocked + chol_solve_blocked, 1024 / 512 threads, nb <= 21, reps ignored, usec5 not written). */
int vio_stage_chol(int nb, int reps, int blocks, const double *S, const double *rhs, double *L_out, double *x_out, double *usec5);
/* Harness of the HBM-resident symmetric eigen-solver of the literal marginalisation (marg_exact = 1, blocks beyond the LDS-resident size: Householder
 * tridiagonalisation + implicit QL by one workgroup, be_linalg.h sym_eig_hbm; Eigen::SelfAdjointEigenSolver at marginalization_factor.cpp:281, :298 is
 * what it stands in for).  A: symmetric n x n, row-major, 2 <= n <= 512.  evals[n] unsorted, evecs[i * n + k] = component i of the eigenvector of
 * evals[k], usec (may be NULL; FOUR doubles) = device time of the decomposition and of its tridiagonalisation / accumulation / QL phases. */
int vio_stage_sym_eig(int n, const double *A, double *evals, double *evecs, double *usec);
/* Harnesses of the other dense primitives of be_linalg.h (stage_linalg.hip), each called directly by one workgroup; VIO_EINVAL for arguments the routine
 * does not support.  Eigenvectors out as in vio_stage_sym_eig: evecs[i * n + k] = component i of the eigenvector of evals[k] (unsorted).
 * vio_stage_jacobi: mode 0 = jacobi_small (thread 0, n <= 16, A / V in LDS), 1 = jacobi_block (A / V in LDS for n <= 96, in HBM beyond, n <= 256),
 * 2 = jacobi_wave16 (wavefront 0, n <= 16, LDS), 3 = jacobi_block with A / V in HBM (as marg_exact runs it).  nt = threads of the workgroup (a
 * multiple of 64, <= 1024).  sweeps_out (may be NULL) = sweeps the routine ran, 0 for mode 0 (jacobi_small does not report them). */
int vio_stage_jacobi(int mode, int n, int nt, const double *A, double *evals, double *evecs, int *sweeps_out);
/* sym_eig_tridiag (one_wave) or sym_eig_tridiag_mt, then tridiag_ql_wave, exactly as be_prior_factor_kernel calls them (512 threads; the matrix in
 * LDS with leading dimension n | 1, or in HBM with n when in_hbm).  1 <= n <= 128.  Only the lower triangle of A is read. */
int vio_stage_sym_eig_lds(int n, int one_wave, int in_hbm, const double *A, double *evals, double *evecs);
/* spd_inverse_wave16 (n <= 16, wavefront 0 of a 512-thread workgroup): ok_out = the routine's result (factorisation succeeded and the eigenvalues are
 * certified above floor), Ainv = A^-1 when ok_out is 1, NaN otherwise. */
int vio_stage_spd_inverse16(int n, double floor, const double *A, double *Ainv, int *ok_out);
/* block_scan_flags on flags[n] (0 / 1) with nt threads (a multiple of 64, <= 1024): offs = exclusive prefix sums, total_out[0] = the total.  skew & 3:
 * 1 / 2 = thread 0 / the last thread starts the scan a few microseconds late; skew & 4: the flags are written just before the call by other threads
 * behind a barrier, as the callers do; skew & 8: two scans back to back on the same scratch, the second into offs[n .. 2 n) (offs holds 2 n) and its
 * total into total_out[1].  total_out[2] = 1 if the LDS words after the routine's 2 nt + 2 scratch ints kept their values.  total_out: 3 ints. */
int vio_stage_scan_flags(int n, int nt, int skew, const int *flags, int *offs, int *total_out);
/* The landmark Schur complement of be_solve: S = S_p H S_p + mu diag(dgp^2) - sum_k inv[k] (S_p Ws[k])^T (S_p Ws[k]) on its lower 16 x 16 tiles, n = 16 nb
 * (nb <= 21), H n x n and Ws Kpad x n row-major (Kpad a multiple of 4), S_p = diag(sp); a column with sp = 0 becomes an identity row.  variant 0 =
 * schur_mfma (S in HBM), 1 = schur_mfma_lds, 2 = schur_mfma_staged<9> with column-tile mask colmask (bit c: column tile c of Ws may be non-zero;
 * only where be_solve would stage, schur_staged_ok), both in an LDS tile region of be_solve's size followed by guard words (guard_ok = 1 if they
 * survived) and untiled into S_out.  nt threads.  S_out: only the lower tiles are written (diagonal tiles whole). */
int vio_stage_schur(int variant, int nb, int nt, int Kpad, unsigned colmask, const double *H, const double *Ws, const double *inv, const double *dgp,
                    const double *sp, double mu, double *S_out, int *guard_ok);
/* be_marg's truncated pseudo-inverse (be_linalg.h marg_pinv15, n <= 15): Pinv of the symmetrised A with eigenvalues <= 1e-8 dropped; path_out = 0 if
 * the certified inverse served (every eigenvalue provably above 1e-6), 1 if the Jacobi eigen-decomposition did. */
int vio_stage_pinv15(int n, const double *A, double *Pinv, int *path_out);
/* One part of the literal marginalisation (vio_config.marg_exact = 1 / 2; be_kernels.hip marg_exact_finish, marg_literal_prior, marg_certificate) on
 * caller-supplied data, as be_marg_exact_kernel runs it: one workgroup of nt threads (256 or 512), the same dynamic LDS.  md = 6 or 15 (pose /
 * pose + speed-bias of frame 0), F0 = 0 .. 480 landmarks in the marginalised block (m = md + F0), n = 1 .. 6 VIO_MAXW + 16 kept parameters.
 * mxl: the largest block whose eigen-decomposition runs LDS-resident; 0 = what a handle chooses (DevCfg::MXL), 1 .. 128 forces the switch to the
 * HBM solver at that size.  All matrices row-major.
 *   part 0  marg_exact_finish.  In: A (mq x mq, mq = md + n, nothing eliminated; only its md x md block is symmetrised), b (mq), Cl (F0 x ldc, the
 *           landmarks' coupling rows, columns indexed like A's; ldc >= mq), Hll = d (F0), gl (F0), second_new (recorded in dbg[2]).
 *           Out: Ainv_out = A_mm^+ (m x m), Ar_out (n x n), br_out (n), and everything part 1 returns.
 *   part 1  marg_literal_prior.  In: A = A_r (n x n), b = b_r (n).  Out: J_out (n x n, row k = sqrt(lambda_k) v_k^T or zero), rf_out (n), H_out = J^T J
 *           (n x n), r_out = J^T rf (n), scal2_out[0] = |rf|^2.
 *   part 2  marg_certificate.  In: A = Pinv (md x md), pinv_direct, second_new, Cl (F0 x ldc, ldc >= md), Hll = 1 / d or 0 (F0).
 *           Out: info8_out[2] = certified, scal2_out[1] = the bound on |A_mm^-1|_F.
 * Pointers a part does not use may be NULL.  info8_out: [0] the effective mxl, [1] 1 if the guard words around every array the kernel may write
 * kept their values, [2] certified (part 2), [3] [4] [5] BeSeq::dbg[0], [2], [4] after the call (-1 = not written; part 0 writes 0, second_new, m).
 * VIO_EINVAL for any other argument and when the kernel's LDS would not fit a workgroup. */
int vio_stage_marg_literal(int part, int md, int F0, int n, int ldc, int nt, int mxl, int pinv_direct, int second_new, const double *A, const double *b,
                           const double *Cl, const double *Hll, const double *gl, double *Ainv_out, double *Ar_out, double *br_out, double *J_out,
                           double *rf_out, double *H_out, double *r_out, double *scal2_out, int *info8_out);
/* The DEFAULT marginalisation (marg_exact = 0) on a caller-chosen state, through the kernels a handle really launches (tests/test_gpu_marg_default.py).
 * vio_debug_marg_set writes one sequence's pre-marginalisation state into the handle's own arrays, vio_debug_marg_run launches what vio_feed launches
 * behind the solve (be_marg_kernel, be_marg_hbm_kernel or be_marg_pre_kernel + be_marg_alg_kernel, with the handle's thread count and dynamic LDS) and
 * waits, vio_debug_marg_get reads the result.  W = window_size, n = 6 W + 16, NL = the handle's landmark capacity (vio_get_capacity).
 * vio_marg_stage_in: t = the tables of vio_stage_publish (lm_order: the first n_lm entries are the live slots in list order, all distinct and < NL; the
 * other tables are indexed by slot and passed whole, [NL]); lm_est_flag [NL]; Vs / Bas / Bgs [W+1][3]; g [3]; prior_present [W+3], prior_H [n][n],
 * prior_r [n], prior_x0 [7 W + 17] (read when has_prior; otherwise the prior is cleared); pre_idx [W+1] = a permutation of 0 .. W (window slot ->
 * pre-integration record).  IMU (read when the handle has use_imu): for the interval that ends in window frame j = 1 .. W, imu_n[j] <= 64 samples
 * imu_dt [W+1][64], imu_acc / imu_gyr [W+1][64][3] (row j), the sample before the first imu_acc0 / imu_gyr0 [W+1][3] and the linearisation biases
 * imu_ba / imu_bg [W+1][3]; they are propagated on the device by the pipeline's routine (vio_stage_preint mode 2, with the sequence's noise
 * densities) into record pre_idx[j], whitening matrix included.  Row 0 of every IMU array is ignored.
 * set also writes frame_count = W, do_marg = 1, rebooted = 0, processed = 0 (so be_finish, fused into the same kernels, leaves the staged window
 * alone: the slide is not part of this harness) and derives lm_free / n_free.  It validates everything a kernel indexes with BEFORE anything is
 * written and returns VIO_EINVAL with vio_last_error set: a slot >= NL or listed twice, n_lm outside 0 .. NL, lm_start outside 0 .. W, lm_nobs outside
 * 1 .. W + 1 - lm_start, more than 64 samples in an interval, Headers not increasing, a depth (or any other number handed over) that is not
 * finite, more landmarks starting in frame 0 than NRES / W residual records hold, pre_idx not a permutation, ring_base outside 0 .. W,
 * marginalization_flag or has_prior not 0 / 1, a handle with marg_exact.  Sequences that were not staged keep do_marg as it was (0 on a fresh handle). */
typedef struct vio_marg_stage_in {
    vio_publish_tables t;
    const int32_t *lm_est_flag;
    int32_t n_lm, ring_base, marginalization_flag, has_prior;
    const double *Vs, *Bas, *Bgs, *g;
    double td;
    const int32_t *prior_present;
    const double *prior_H, *prior_r, *prior_x0;
    const int32_t *pre_idx;
    const int32_t *imu_n;
    const double *imu_dt, *imu_acc, *imu_gyr, *imu_acc0, *imu_gyr0, *imu_ba, *imu_bg;
} vio_marg_stage_in;
/* vio_marg_stage_out (every pointer may be NULL): prior_H [n][n], prior_r [n], prior_x0 [7 W + 17], prior_present [W+3], prior_c0 [1], has_prior [1],
 * dbg5 = BeSeq::dbg[0 .. 4]; and what survives in HBM where the handle runs be_marg_hbm_kernel (hbm_valid[0] = 1; otherwise 0 and the four are left
 * as passed in): margA [(15 + n)^2] = the reduced system over q = [m-block (md = 15, or 6 for MARGIN_SECOND_NEW) | kept (n)] after the landmarks are
 * eliminated, row-major with leading dimension md + n in the first (md + n)^2 doubles, margB [15 + n] its right-hand side (first md + n), margV [n][n]
 * = A_r, b_r [n]. */
typedef struct vio_marg_stage_out {
    double *prior_H, *prior_r, *prior_x0;
    int32_t *prior_present;
    double *prior_c0;
    int32_t *has_prior, *dbg5;
    double *margA, *margB, *margV, *b_r;
    int32_t *hbm_valid;
} vio_marg_stage_out;
int vio_debug_marg_set(vio_batch *h, int seq, const vio_marg_stage_in *in);
int vio_debug_marg_run(vio_batch *h);
int vio_debug_marg_get(vio_batch *h, int seq, vio_marg_stage_out *out);
/* The SOLVER on a caller-chosen state, launch by launch, through the kernels a handle really launches (tests/test_gpu_solve_stage.py).
 * vio_debug_solve_set takes the input of vio_debug_marg_set through the same validation and writes the same state, with do_solve = 1,
 * solver_flag = 1, do_marg = 0, openExEstimation = 0, no relocalisation request, init_frame = 0 and last_P / last_R (what failureDetection
 * compares the solved window with) = the staged newest frame, as a processed frame leaves them.  It refuses in addition, with VIO_EINVAL and
 * nothing written, what the solver indexes with and the marginalisation does not: lm_est_flag of a live slot outside 0 .. 2; more projection
 * residuals (sum of lm_nobs - 1 over the landmarks in the problem: !lm_dyn, lm_nobs >= 2, lm_start < W - 2) than the residual list holds
 * (NRES - 2 NL records) or, on a phased handle, than its evaluation launch covers (landmarks in the problem cannot exceed NL once the list is
 * valid).  marginalization_flag
 * is stored and otherwise ignored.
 * vio_debug_solve_run(h, slots, stop_phase, radius0), slots >= 0: ps_setup, `slots` whole slots (evaluate [+ accept], assemble, Schur, serial, line
 * search), then the kernels of one more slot up to and including stop_phase, then it waits; no ps_final, so the staged window stays as it is and
 * the state can be run again.  radius0 > 0 overwrites SolveSt::radius by a copy between ps_setup and the first slot -- the only state the harness
 * touches itself; the copy goes to the sequences vio_debug_solve_set has staged on this handle and to no other (an idle sequence's snapshot stays as it is).  slots + (stop_phase != NONE) may not exceed max_iterations + the handle's extra slots.  slots < 0: the whole solve with
 * ps_final (or the persistent kernel), the launches of vio_feed on the back-end stream (stop_phase and radius0 must be 0); the only form a
 * handle without the phased solver (VIO_SOLVE_MODE=0, or a configuration it does not cover) accepts.
 * vio_debug_solve_get (every pointer may be NULL; P = 15 (W + 1) + 7, parameter order pose k at 6 k, speed-bias k at 6 (W + 1) + 9 k, extrinsic at
 * 15 (W + 1), td at 15 (W + 1) + 6; F, Fa = landmarks in the problem / variable ones; phased handles only, VIO_EINVAL otherwise):
 *   always (after ps_setup)      scal_i [11] = stage iter iters_done F Fa nres ex_active td_active vext constrained fused; scal_d [7] = cost ccost
 *                                radius mu alpha dogleg_norm model_change; X [16 (W + 1) + 8] = pose [W+1][7], speed-bias [W+1][9], extrinsic [7], td;
 *                                feat [NL] (first F: inverse depths in list order); var_slots [NL] (first Fa: landmark slots in solver order)
 *                                (ccost = the partial costs of the last evaluation, SolveSt::part, summed in index order: the kernels keep the
 *                                candidate's cost in a register and never write SolveSt::ccost)
 *   after VIO_SOLVE_STOP_ASM_A   cost (slot 0) or ccost, the accept / reject decision and the new radius (later slots); Hpl [NL][P] (first Fa rows;
 *                                columns of poses and, with vext, of extrinsic and td -- every other column is returned as 0, the kernels leave
 *                                them unwritten), Hll, gl [NL] of the CURRENT point (X, feat), unscaled
 *   after VIO_SOLVE_STOP_SCHUR   H [P][P] (full, symmetric, unscaled), g [P], sp [P] (Jacobi column scaling, 0 = constant parameter); Sc [LW][LW]
 *                                (LW = P rounded up to 16): the lower 16 x 16 tiles untiled, 0 above them.  While the column scaling is being fixed
 *                                (the first linearisation of a solve, and Cholesky retries) the tiles hold U = sum_k w_k h_k h_k^T, the landmark part
 *                                of the Schur complement, in the tiles the landmark rows touch only (the others are stale); afterwards all of them
 *                                hold S = Sp (H - U) Sp + mu D^2 with unit diagonal for constant and padding parameters
 *   after VIO_SOLVE_STOP_SERIAL  sl [NL], dgp [P] / dgl [NL] (trust-region diagonal D), gnp / gnl (Gauss-Newton step, D-scaled: - D y), stp / stl
 *                                (dogleg step in the Jacobi-scaled variables: x step = sp stp, sl stl), alpha, dogleg_norm, model_change, Xc and
 *                                cfeat (the candidate); on windows beyond W = 10 Sc then holds the Cholesky factor
 *   after VIO_SOLVE_STOP_LS      Xc, cfeat: the candidate the projected line search of a bounds-constrained solve settled on
 * Landmark vectors are indexed by solver order (var_slots), the first Fa entries. */
enum { VIO_SOLVE_STOP_NONE = 0, VIO_SOLVE_STOP_ASM_A = 1, VIO_SOLVE_STOP_SCHUR = 2, VIO_SOLVE_STOP_SERIAL = 3, VIO_SOLVE_STOP_LS = 4 };
typedef struct vio_solve_stage_out {
    int32_t *scal_i;
    double *scal_d;
    double *X, *Xc, *feat, *cfeat;
    int32_t *var_slots;
    double *H, *g, *sp;
    double *Hpl, *Hll, *gl, *sl;
    double *Sc;
    double *dgp, *dgl, *gnp, *gnl, *stp, *stl;
} vio_solve_stage_out;
int vio_debug_solve_set(vio_batch *h, int seq, const vio_marg_stage_in *in);
int vio_debug_solve_run(vio_batch *h, int slots, int stop_phase, double radius0);
int vio_debug_solve_get(vio_batch *h, int seq, vio_solve_stage_out *out);

#ifdef __cplusplus
}
#endif
#endif
