// The handle behind the C ABI (include/vio_abi.h) and what its host translation units share: struct vio_batch, the table of its device arrays,
// the ownership helpers, the prologue of an entry point and the LDS / environment helpers.  vio_abi.hip creates, destroys and feeds a handle,
// abi_query.hip reads and sets it between frames, abi_snapshot.hip saves and restores its sequences.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <stdlib.h>
#include <mutex>
#include <chrono>
#include <string>
#include <string.h>
#include <vector>
#include "kernels.h"
#include "dyninit_host.h"
#include "camera_model.h"
#include "snapshot.h"
#include "stage_util.h"

struct vio_batch {
    DevCfg hc;  // host copy
    Batch B;
    int S;
    int device = -1;   // the HIP device this handle's memory, streams and events live on (vio_create: the caller's current device; vio_create_on_device:
                       // the one asked for).  Every entry point binds the calling thread to it for the duration of the call (DevGuard below).
    // Sequences are split into groups of contiguous sequences; every group has its own pair of streams, so the chain
    // track -> ingest -> solve -> marginalise of one group never waits for the slowest sequence of another group.
    struct Group {
        int s0 = 0, n = 0;
        hipStream_t stream = nullptr;     // back-end (and uploads that feed it)
        hipStream_t fe_stream = nullptr;  // front-end: frame k+1 tracks while frame k is still being marginalised
        hipEvent_t ev_solve = nullptr, ev_fe = nullptr, ev_be = nullptr, ev_ingest = nullptr;
        hipStream_t copy_stream = nullptr;   // host -> HBM uploads of vio_feed (on_device == 0), beside the kernels of the previous frame
        hipStream_t copy_stream2 = nullptr;  // the depth images on a stream of their own: two DMA engines per group (one stream moves ~25 GB/s from page-locked memory)
        // vio_feed uploads from host buffers: one event pair per staging buffer (g.flip), so that TWO uploads may be in flight -- the call that
        // reuses a staging buffer waits for the upload of two calls ago, not for the previous one (round 5; vio_host_buffers_done)
        hipEvent_t ev_up_gray[2] = {nullptr, nullptr}, ev_up_depth[2] = {nullptr, nullptr};
        bool up_used[2] = {false, false};
        // the staging images of vio_feed are double-buffered: frame n uploads into buffer n & 1 while frame n-1's kernels still read the
        // other one, so an upload only waits for the readers of frame n-2 (ev_rd_gray / ev_rd_depth of its buffer)
        int flip = 0;
        hipEvent_t ev_rd_gray[2] = {nullptr, nullptr}, ev_rd_depth[2] = {nullptr, nullptr};
        bool have_rd_gray[2] = {false, false}, have_rd_depth[2] = {false, false};
        // host -> HBM uploads enqueued on fe_stream / stream by the non-overlap entry points (vio_track, vio_process, vio_process_obs*):
        // asynchronous when the caller's buffers are page-locked, so the next call that takes host buffers waits for them first
        hipEvent_t ev_host_fe = nullptr, ev_host_be = nullptr;
        bool host_fe_pending = false, host_be_pending = false;
        bool have_solve_ev = false, have_ingest_ev = false;
        // ev_slide: the window slide of the last frame has run (recorded behind the kernel that holds finish_body, whichever it is); ev_setup: be_ingest
        // and ps_setup of a frame that ran them on fe_stream (VIO_MARG_SPLIT) are done
        hipEvent_t ev_slide = nullptr, ev_setup = nullptr;
        bool have_slide_ev = false;
        hipEvent_t depth_wait = nullptr;   // the depth upload this call's be_ingest on fe_stream still has to wait for (stage_inputs -> launch_backend)
        // vio_feed: stamps / frame modes of a call bounce through a library-owned page-locked ring, so the caller's arrays are free when the
        // call returns although the copies only run when fe_stream gets to them (tracker lag 1 holds that stream behind be_ingest)
        static constexpr int kSideRing = 16;
        unsigned char *side_ring = nullptr;          // [kSideRing][n * 9]: n doubles then n mode bytes
        hipEvent_t side_ev[kSideRing] = {};
        bool side_used[kSideRing] = {};
        int side_pos = 0;
    };
    std::vector<Group> groups;
    int tracker_lag = 0;              // vio_set_tracker_lag
    int extra_slots = 2;              // VIO_EXTRA_SLOTS: iteration slots beyond max_iterations (1 carries the last evaluation, the second absorbs one Cholesky retry / invalid step)
    int xcd_map = 1;                  // VIO_XCD_MAP: XCD-aware block map of the multi-block ps_* kernels (be_phased.h ps_blk)
    int fe_xcd_map = 1;               // VIO_FE_XCD_MAP: the same idea for fe_lk (needs the front-end on every XCD: off under a CU partition)
    bool fe_partitioned = false;      // the front-end streams carry a CU mask (VIO_FE_CUS > 0 with tracker lag 1)
    int ps_asm_b_blocks = 24;         // workgroups per sequence that sum the entries of H (VIO_ASM_B_BLOCKS)
    hipStream_t stream = nullptr;     // = groups[0].stream (returned by vio_get_stream; IMU scatter runs here)
    hipStream_t fe_stream = nullptr;  // = groups[0].fe_stream
    hipEvent_t ev[4];
    // what the handle owns, by kind, filled where a thing is created (dev_alloc / pinned_alloc / new_event / own_stream below): vio_destroy
    // releases these four lists and nothing else
    std::vector<void *> allocs, pinned;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
    uint8_t *d_fisheye = nullptr;                                    // vio_set_fisheye_mask
    uint8_t *d_gray_stage = nullptr, *d_gray_stage1 = nullptr;       // [S][H][W] staging images of host-buffer calls; the second one only for vio_feed
    uint16_t *d_depth_stage = nullptr, *d_depth_stage1 = nullptr;
    double *d_stamps = nullptr;
    uint8_t *d_modes = nullptr;       // [S] frame modes of the current vio_feed_modes / vio_track_ex call
    double *d_rrel = nullptr;         // [S][9] caller-supplied relative rotations (vio_track_ex)
    // caller-supplied feature maps (vio_process_obs): [S] counts / stamps, [S][NP] ids, [S][NP][7] observations
    int *d_in_n = nullptr, *d_in_ids = nullptr;
    double *d_in_obs = nullptr, *d_in_stamps = nullptr;
    double *d_r9 = nullptr;           // vio_predict_motion result
    // vio_get_latest_odometry_all / vio_get_imu_rate_odometry: per-call device staging (since [S], n_rows [S], last [S][11], rows [S][cap][11])
    // and its page-locked host image, both grown on demand
    double *d_odo = nullptr, *h_odo = nullptr;
    size_t odo_cap = 0, h_odo_cap = 0;
    // vio_publish_all: the same pair for the publishers (counts [S][4], kf_pose [S][8], then the row lists of a host destination)
    double *d_pub = nullptr, *h_pub = nullptr;
    size_t pub_cap = 0, h_pub_cap = 0;
    // per-sequence calibration (vio_set_calibration): host mirror of the device table B.cal, as in effect (ric re-orthonormalised, I / 0 on
    // estimate_extrinsic = 2 handles)
    std::vector<vio_calibration> cal;
    vio_calibration *d_cal = nullptr;
    // per-sequence camera model (vio_set_camera): host mirror of the device table (cam_of, after B.cal).  A PINHOLE slot's parameters live in cal (vio_get_camera reads them there)
    std::vector<vio_camera> cam;
    vio_camera *d_cam = nullptr;
    // ---- dynamic initialisation (static_init: 0): host mirror of Estimator::all_image_frame per sequence while it is INITIAL
    struct DynSeq {
        std::vector<vinit::ImageFrame> frames;
        double initial_timestamp = 0;
        bool nonlinear = false;       // host view of solver_flag (refreshed from h_state)
        int attempts = 0, failures = 0, last_stage = 0;
    };
    std::vector<DynSeq> dyn;          // [S], only used when cfg.dynamic_init
    bool dyn_active = false;          // some sequence is still INITIAL: the back-end runs in two halves with the host in between
    int *h_state = nullptr;           // pinned [S]: solver_flag of every sequence after the last be_solve (async copy per frame)
    int *d_state = nullptr;
    hipEvent_t ev_state = nullptr;
    bool state_pending = false;
    double *d_dyn_samples = nullptr;  // IMU steps of the window slots handed to be_dyn_finalize_kernel (grown on demand)
    int *d_dyn_offs = nullptr;
    size_t dyn_samples_cap = 0;
    // pending IMU samples (host staging)
    std::mutex imu_mu;
    std::vector<int> p_seq;
    std::vector<double> p_t, p_acc, p_gyr;
    // IMU upload: two pinned host staging sets + device sets used alternately, each guarded by an event, so that vio_push_imu
    // between frames never forces a device-wide synchronisation (the scatter kernel is ordered on the streams instead)
    struct ImuStage {
        int *h_seq = nullptr, *d_seq = nullptr;
        double *h_t = nullptr, *h_acc = nullptr, *h_gyr = nullptr, *d_t = nullptr, *d_acc = nullptr, *d_gyr = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    } imu_stage[2];
    int imu_stage_cur = 0;
    hipEvent_t ev_imu = nullptr;
    std::vector<double> last_imu_t;
    size_t lds_select = 0, lds_add = 0, lds_fast = 0, lds_solve = 0, lds_serial = 0, lds_marg = 0, lds_factor = 0, lds_ps_ls = 0, lds_ps_evalf = 0;
    int ps_evalf_blocks = 0;           // workgroups per sequence of ps_evalf_kernel (2 + B.fuse)
    bool feed_throttle = true;         // VIO_FEED_THROTTLE: host-fed vio_feed waits for the back-end of two feeds ago before it enqueues (stage_inputs)
    int uploads_in_flight = 2;         // VIO_UPLOADS_IN_FLIGHT: page-locked image uploads of vio_feed that may be pending when a call returns
    int relo_frames = 0;               // frames for which the two-kernel solver path is launched beside the fused kernel (armed by vio_set_relo_frame)
    bool line_search = true;           // ps_ls_kernel behind every ps_serial (Ceres' projected line search on bounds-constrained solves)
    // VIO_BE_THREADS / VIO_MARG_THREADS, read at vio_create.  The marginalisation kernel runs next to the following frame's front-end:
    // with 6 instead of 8 wavefronts (256 VGPRs each) two SIMDs per CU keep half of their register file free and the LK wavefronts can
    // co-reside (be_marg 1.4 -> 1.6 ms, fe_lk 0.77 -> 0.60 ms; the front-end is the longer of the two, so the step gets shorter).
    int be_threads = 512, marg_threads = 384;
    // VIO_MARG_LDS (default 1): be_marg keeps its reduced system, frame blocks and landmark tables in LDS where they fit (size_launches decides: W = 10
    // does, W = 12 and up do not); false = be_marg_hbm_kernel, the HBM scratch of rounds 1 - 6
    bool marg_lds = true;
    // VIO_PREINT_AHEAD (default 1): vio_feed pre-integrates a frame's IMU interval on the front-end stream beside be_marg of the previous frame
    // (be_preint_ahead_kernel) and be_ingest takes the result over where its inputs still hold; false = never launched, be_ingest integrates itself.
    // d_ahead: the [S] records, a per-call buffer like d_stamps (allocated at vio_create where the knob is on and the handle has an IMU)
    bool preint_ahead = true;
    PreAhead *d_ahead = nullptr;
    // VIO_MARG_SPLIT (default 1): vio_feed launches the marginalisation as be_marg_pre_kernel + be_marg_alg_kernel (kernels.h) and runs the NEXT frame's
    // be_ingest and ps_setup on the group's front-end stream behind the first of them (Group::ev_slide), beside the second; the back-end stream picks
    // the frame up at its first solver slot (Group::ev_setup).  Taken where the phased solver, the default marginalisation in LDS, an IMU, tracker lag 1
    // and a whole-group feed come together and the handle does not initialise dynamically (vio_abi.hip split_feed); 0 = the one be_marg launch and the
    // one-stream order everywhere.  d_msnap / d_mlist: the hand-over between the two kernels, per-call buffers like d_ahead.
    bool marg_split = true;
    MargSnap *d_msnap = nullptr;
    int *d_mlist = nullptr;
    // VIO_SOLVE_MODE: 0 = persistent kernel (one workgroup per sequence for the whole solve), 1 = phased solver (be_phased.h, default)
    int solve_mode = 1;
    std::vector<char> solve_staged;   // [S] vio_debug_solve_set has staged the sequence: the only ones whose SolveSt::radius vio_debug_solve_run may write
    bool serial_big = false;          // the window's Schur complement does not fit LDS: ps_serial_big_kernel (HBM-resident tiles, streaming Cholesky)
    size_t lds_ps_eval = 0;
    int ps_eval_blocks = 0, ps_asm_a_blocks = 0, ps_schur_tiles = 0;
    bool timing_valid = false;
    // per-kernel event pool (vio_profile_begin / vio_profile_end)
    std::vector<hipEvent_t> pev;
    int prof_steps = 0, prof_cur = -1;
    bool prof_fe_only = false;        // the profiled steps were vio_track calls: only the front-end events exist
    // sequence snapshots (vio_save_seqs / vio_load_seqs): the layout table (built at the first use), its device copy, the sequence list of a call
    // and the staging buffer the pack / unpack kernels work on.  Nothing of this is allocated until the first save or load.
    struct SnapRow { const char *name; int kind; unsigned char *base; int64_t bytes, blob_off; };   // kind: 1 state, 0 scratch, 2 handle-wide (not per sequence)
    std::vector<SnapRow> snap_rows;
    int64_t snap_dev_bytes = 0, snap_chunks = 0;
    int snap_entries = 0;
    SnapEntry *d_snap_tab = nullptr;
    SnapSeq *d_snap_seqs = nullptr;
    size_t snap_seqs_cap = 0;
    unsigned char *d_snap_stage = nullptr;
    size_t snap_stage_cap = 0;
};
#define VIO_NK 10  // kernels per vio_feed: fe_begin pyrdown predict lk select fast add | be_ingest solve marg(+finish)
#define VIO_NEV 12 // events per step: 0..7 bracket the front-end kernels on fe_stream, 8..11 the back-end kernels on stream
#define PEV_ON(h, k, strm) do { if (g.s0 == 0 && (h)->prof_cur >= 0 && (h)->prof_cur < (h)->prof_steps) (void)hipEventRecord((h)->pev[(size_t)(h)->prof_cur * VIO_NEV + (k)], (strm)); } while (0)   // the same, on the stream the bracketed kernel runs on
#define PEV(h, k) do { if (g.s0 == 0 && (h)->prof_cur >= 0 && (h)->prof_cur < (h)->prof_steps) (void)hipEventRecord((h)->pev[(size_t)(h)->prof_cur * VIO_NEV + (k)], (k) <= 7 ? g.fe_stream : g.stream); } while (0)

// an integer knob from the environment (clamps stay with the caller)
inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel, not of a handle: with several handles of different
// configurations alive, keep the largest value ever requested (monotonic), otherwise the handle created last would shrink the
// limit under the others.
inline int raise_lds_limit(const void *fn, size_t bytes) {
    // the attribute belongs to the function ON THE CURRENT DEVICE (a handle per GPU in one process sets it once per device)
    struct Seen { const void *fn; int dev; size_t bytes; };
    static std::mutex mu;
    static std::vector<Seen> seen;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : seen)
        if (e.fn == fn && e.dev == dev && bytes <= e.bytes) return 0;
    // a size the runtime refuses is not remembered, and its error is taken off the thread: the callers decide with lds_fits, and an
    // error left behind would be reported by the next entry point that ends with hipGetLastError()
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (auto &e : seen)
        if (e.fn == fn && e.dev == dev) { e.bytes = bytes; return 0; }
    seen.push_back({fn, dev, bytes});
    return 0;
}

// static + dynamic LDS of a kernel this handle will launch against what a workgroup may own: a configuration that does not fit fails at
// vio_create, not with an aborted launch in the middle of a frame
inline bool lds_fits(const void *fn, size_t dynamic_bytes, const char *name) {
    hipFuncAttributes a;
    int dev = 0, cap = 0;
    if (hipFuncGetAttributes(&a, fn) != hipSuccess) return true;   // (cannot tell: let the launch decide)
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || cap <= 0) cap = 160 * 1024;
    if (a.sharedSizeBytes + dynamic_bytes <= (size_t)cap) return true;
    g_err = std::string("configuration needs more LDS than a workgroup may own: ") + name;
    return false;
}

// marg_exact: the eigen-decompositions of the literal marginalisation run LDS-resident for blocks up to MXL (DevCfg::MXL) -- whatever
// be_marg_exact_kernel's static LDS leaves of the workgroup's share (matrix with an odd leading dimension + the solver's vectors, be_kernels.hip
// MARG_EIG_AUX_DOUBLES), and never beyond the 128 rows tridiag_ql_wave covers.  0 when the kernel's attributes cannot be read.
inline int marg_exact_mxl(int device) {
    hipFuncAttributes fa;
    int cap = 0;
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || cap <= 0) cap = 160 * 1024;
    if (hipFuncGetAttributes(&fa, (const void *)be_marg_exact_kernel) != hipSuccess) return 0;
    const long avail = (long)cap - (long)fa.sharedSizeBytes - 256;
    int m = 0;
    while (m < 128 && (long)marg_exact_lds_bytes(m + 1) <= avail) m++;
    return m;
}

// A handle owns its device: entry points may be called from any host thread with any device current (one host thread per GPU
// in one process, or a caller that moves between devices); the guard makes h->device current for the call and restores the caller's on return.
struct DevGuard {
    int prev = -1;
    bool switched = false;
    bool failed = false;   // the handle's device could not be made current: the entry point must not run on the caller's device instead
    explicit DevGuard(const vio_batch *h) {
        if (!h || h->device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) { failed = true; return; }
        if (prev != h->device) { switched = hipSetDevice(h->device) == hipSuccess; failed = !switched; }
    }
    ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};
inline int sync_all(vio_batch *h) {
    for (auto &g : h->groups) {
        if (g.copy_stream) HIPCHK(hipStreamSynchronize(g.copy_stream));
        if (g.copy_stream2) HIPCHK(hipStreamSynchronize(g.copy_stream2));
        HIPCHK(hipStreamSynchronize(g.fe_stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        g.host_fe_pending = g.host_be_pending = false;
    }
    return VIO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- entry-point prologue
// VIO_ENTER(h, seq, sync) opens every extern "C" function that takes a handle: it binds the calling thread to the handle's device for the
// call (dev_guard), returns VIO_EDEVICE when that failed -- the function must not run on the caller's device with another device's
// pointers --, VIO_EINVAL for a null handle or a seq outside [0, S) (VIO_NO_SEQ: the function takes none), and, with sync, waits for
// everything the handle has enqueued.  VIO_ENTER_MSG also leaves `msg` in vio_last_error on VIO_EINVAL.
enum { VIO_NO_SEQ = INT_MIN };
inline int vio_enter(const DevGuard &guard, vio_batch *h, int seq, bool sync, const char *einval_msg = nullptr) {
    if (guard.failed) { g_err = "hipSetDevice failed for the handle's device"; return VIO_EDEVICE; }
    if (!h || (seq != VIO_NO_SEQ && (seq < 0 || seq >= h->S))) {
        if (einval_msg) g_err = einval_msg;
        return VIO_EINVAL;
    }
    return sync ? sync_all(h) : VIO_OK;
}
#define VIO_ENTER_MSG(h, seq, sync, msg)                                                      \
    DevGuard dev_guard(h);                                                                    \
    { const int rc_ = vio_enter(dev_guard, h, seq, sync, msg); if (rc_ != VIO_OK) return rc_; }
#define VIO_ENTER(h, seq, sync) VIO_ENTER_MSG(h, seq, sync, nullptr)
#define VIO_TRY(x) { const int rc_ = (x); if (rc_ != VIO_OK) return rc_; }

// ---------------------------------------------------------------------------------------------------------------- ownership
// Whatever a handle creates goes through one of these, which files it in the list of its kind; a buffer that is regrown is released
// through the matching *_release, so that no stale pointer stays in a list.  count == 0: nothing is allocated and *p stays null.
template <class T> int dev_alloc(vio_batch *h, T **p, size_t count, bool zero = true) {
    if (count == 0) return VIO_OK;
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, count * sizeof(T)));
    h->allocs.push_back(q);
    *p = (T *)q;
    if (zero) HIPCHK(hipMemset(q, 0, count * sizeof(T)));
    return VIO_OK;
}
template <class T> int pinned_alloc(vio_batch *h, T **p, size_t count) {
    void *q = nullptr;
    HIPCHK(hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault));
    h->pinned.push_back(q);
    *p = (T *)q;
    return VIO_OK;
}
inline int new_event(vio_batch *h, hipEvent_t *e, unsigned flags = hipEventDisableTiming) {
    HIPCHK(hipEventCreateWithFlags(e, flags));
    h->events.push_back(*e);
    return VIO_OK;
}
inline void own_stream(vio_batch *h, hipStream_t s) { h->streams.push_back(s); }
template <class V, class P> void disown(V &list, P p) { list.erase(std::remove(list.begin(), list.end(), p), list.end()); }
template <class T> void dev_release(vio_batch *h, T *&p) { if (p) { disown(h->allocs, (void *)p); (void)hipFree(p); p = nullptr; } }
template <class T> void pinned_release(vio_batch *h, T *&p) { if (p) { disown(h->pinned, (void *)p); (void)hipHostFree(p); p = nullptr; } }
inline void stream_release(vio_batch *h, hipStream_t &s) { if (s) { disown(h->streams, s); (void)hipStreamDestroy(s); s = nullptr; } }

// ---------------------------------------------------------------------------------------------------------------- the array table
// THE TABLE OF THE HANDLE'S DEVICE ARRAYS: every member of Batch, DevCfg::exc / exh and every per-sequence host vector of vio_batch, declared
// once with its kind and its element count per sequence.  vio_create_on_device allocates by walking it (handle_alloc_arrays), the snapshot
// code builds its rows by walking it (snapshot_build_layout, abi_snapshot.hip: vio_save_seqs, vio_load_seqs, the naive reference loop and
// vio_debug_snapshot_layout).  Assigning a pointer member of Batch anywhere else is an error -- with ONE exception, B.fisheye, which
// vio_set_fisheye_mask sets.  A new array must be given a kind here before it can be allocated at all:
//   STATE    what a snapshot carries: the blob's device part is the STATE rows in table order, each at the next multiple of 16 bytes
//   SCRATCH  rewritten by every frame before it is read
//   HANDLE   not per sequence (documentation rows, and the two handle-wide allocations)
// When in doubt an array is state.  The ORDER of the entries is the snapshot format (VIO_SNAPSHOT_FORMAT): do not reorder.
// A count of 0 means "this configuration has no such array": nothing is allocated, the pointer stays null (code tests for that: B.fuse needs
// B.pairpart, DevCfg::exc selects the calibrating ingest) and the row reports 0 bytes.  The per-call input buffers of a handle (d_stamps,
// d_modes, d_rrel, d_r9, d_odo, d_pub, d_in_*, d_ahead) are not per-sequence state and are not in the table.
// Entry forms (the walkers define h, B = h->B, C = h->hc, D = the dimensions below, S = sequences):
//   SEQ(kind, member, count)             Batch member B.member, row named after the member, S * count elements
//   ROW(kind, name, lvalue, count, n)    a per-sequence row over an array that is not a plain Batch member; n elements are allocated in all
//   VIEW(kind, name, lvalue, count, at)  a row over part of another entry's allocation: lvalue = at, nothing is allocated
//   WIDE(name, lvalue, n)                a handle-wide allocation of n elements; a documentation row
//   DOC(name)                            a documentation row for scalar members
//   HOST(kind, name, bytes)              per-sequence host state: travels in the host part of a blob
struct HandleDims {
    int64_t NP, NL, W, W1, HW, n, LW, nres, npair, mq, NIMU, pyr_bytes, ncells, hist_cap, MX;
    int64_t ls_bytes;                  // ps_eval_lds_bytes(W)
    int64_t clahe, fuse_rows, excal;   // 1 where the configuration has the optional arrays (equalize, W <= PS_FUSE_MAXW, estimate_extrinsic = 2), else 0
};
inline HandleDims handle_dims(const DevCfg &C, int hist_cap) {
    HandleDims D;
    D.NP = C.NP; D.NL = C.NL; D.W = C.W; D.W1 = C.W + 1; D.HW = (int64_t)C.c.width * C.c.height; D.n = C.NPRIOR; D.LW = C.LW; D.nres = C.NRES;
    D.npair = D.W1 * D.W1; D.mq = 15 + D.n; D.NIMU = C.NIMU; D.pyr_bytes = C.pyr_bytes; D.ncells = C.ncells; D.hist_cap = hist_cap; D.MX = C.MX;
    D.ls_bytes = (int64_t)ps_eval_lds_bytes(C.W);
    D.clahe = C.c.equalize ? 1 : 0; D.fuse_rows = C.W <= PS_FUSE_MAXW ? 1 : 0; D.excal = C.c.estimate_extrinsic == 2 ? 1 : 0;
    return D;
}
// the camera table follows the calibration table in one allocation (cam_of, vio_state.h)
static_assert(sizeof(vio_calibration) % alignof(vio_camera) == 0, "camera table alignment");
#define VIO_HANDLE_ARRAYS(SEQ, ROW, VIEW, WIDE, DOC, HOST)                                                                                      \
    WIDE("cfg", B.cfg, 1) DOC("S") DOC("s0 ns xcd_nb xcd_n") DOC("tracker_lag (header)") DOC("eval_rpt")                                        \
    SEQ(STATE, fe, 1) SEQ(STATE, be, 1)                                                                                                         \
    /* the slot's vio_calibration and vio_camera: host mirrors vio_batch::cal / cam */                                                          \
    ROW(STATE, "cal", B.cal, 1, S * (sizeof(vio_calibration) + sizeof(vio_camera)) / sizeof(vio_calibration) + 1)                               \
    VIEW(STATE, "cam (cam_of)", h->d_cam, 1, (vio_camera *)(B.cal + S))                                                                         \
    SEQ(STATE, pre, D.W + 2)                                                                                                                    \
    SEQ(STATE, img, 2 * D.HW) SEQ(STATE, pyr, 2 * D.pyr_bytes)                                                                                  \
    SEQ(SCRATCH, clahe_lut, D.clahe * 64 * 256) SEQ(SCRATCH, clahe_img, D.clahe * D.HW)                                                         \
    DOC("fisheye")                                                                                                                              \
    SEQ(STATE, cur_pts, D.NP) SEQ(STATE, forw_pts, D.NP) SEQ(STATE, cur_un_pts, D.NP) SEQ(STATE, pts_velocity, D.NP)                            \
    SEQ(STATE, prev_un_pt, D.NP) SEQ(STATE, unstable_pts, D.NP)                                                                                 \
    SEQ(SCRATCH, tmp_pts, D.NP)                                                                                                                 \
    SEQ(STATE, ids, D.NP) SEQ(STATE, track_cnt, D.NP) SEQ(STATE, prev_un_id, D.NP)                                                              \
    SEQ(SCRATCH, tmp_i0, D.NP) SEQ(SCRATCH, tmp_i1, D.NP)                                                                                       \
    SEQ(STATE, lk_status, D.NP) SEQ(STATE, accept_xy, 2 * D.NP)                                                                                 \
    SEQ(SCRATCH, cand, D.ncells * VIO_FAST_CAP)                                                                                                 \
    SEQ(STATE, obs_id, D.NP) SEQ(STATE, obs, D.NP * 7)                                                                                          \
    SEQ(STATE, imu_t, D.NIMU) SEQ(STATE, imu_acc, D.NIMU * 3) SEQ(STATE, imu_gyr, D.NIMU * 3)                                                   \
    SEQ(STATE, lm_id, D.NL) SEQ(STATE, lm_start, D.NL) SEQ(STATE, lm_nobs, D.NL) SEQ(STATE, lm_est_flag, D.NL)                                  \
    SEQ(STATE, lm_solve_flag, D.NL) SEQ(STATE, lm_dyn, D.NL)                                                                                    \
    SEQ(STATE, lm_order, D.NL) SEQ(STATE, lm_free, D.NL)                                                                                        \
    SEQ(SCRATCH, lm_tmp, D.NL)                                                                                                                  \
    SEQ(STATE, lm_pidx, D.NL) SEQ(STATE, lm_aidx, D.NL)                                                                                         \
    SEQ(STATE, lm_depth, D.NL) SEQ(STATE, lm_obs, D.NL * D.W1 * VIO_OBS_D)                                                                      \
    SEQ(STATE, lm_relo, D.NL) SEQ(STATE, relo_xy, D.NL * 2) SEQ(STATE, relo_mp, D.NP * 3)                                                       \
    SEQ(STATE, para_feat, D.NL)                                                                                                                 \
    SEQ(SCRATCH, cand_feat, D.NL)                                                                                                               \
    SEQ(SCRATCH, prior_J, D.n * D.n) /* the factored form, produced on demand by vio_get_prior */                                               \
    SEQ(STATE, prior_r, D.n) SEQ(STATE, prior_x0, D.W * 7 + 17) SEQ(STATE, prior_H, D.n * D.n)                                                  \
    SEQ(SCRATCH, prior_rf, D.n)                                                                                                                 \
    /* (the landmark rows Hpl / Hll / gl twice: be_phased.h ps_sel_rows -- the fused evaluate + assemble kernel builds a candidate's rows       \
       beside the current ones) */                                                                                                              \
    SEQ(SCRATCH, H, D.LW * D.LW) SEQ(SCRATCH, Sc, D.LW * D.LW) SEQ(SCRATCH, Hpl, 2 * (D.NL + 8) * D.LW) SEQ(SCRATCH, vec, VEC_SLOTS * D.LW)     \
    SEQ(SCRATCH, Hll, 2 * (D.NL + 8)) SEQ(SCRATCH, gl, 2 * (D.NL + 8)) SEQ(SCRATCH, lvec, (D.NL + 8) * 8)                                       \
    SEQ(SCRATCH, res, D.nres * 42) SEQ(SCRATCH, res_pair, 1) SEQ(SCRATCH, res_lm, D.nres) SEQ(SCRATCH, res_k, D.nres)                           \
    SEQ(SCRATCH, pair_start, D.npair + 1) SEQ(SCRATCH, pair_list, D.nres) SEQ(SCRATCH, pairblk, D.npair * 210)                                  \
    SEQ(SCRATCH, ls_scratch, D.ls_bytes) SEQ(SCRATCH, pairpart, D.fuse_rows * PS_FUSE_MAXPAIRS * PS_FUSE_MAXBLK * 210)                          \
    DOC("gW gP gLW gNL gNP gNRES gNPRIOR gMX") DOC("n_schur fuse fuse_only")                                                                    \
    SEQ(SCRATCH, imu_raw, D.W * 15 * 31)                                                                                                        \
    SEQ(SCRATCH, margA, D.mq * D.mq) SEQ(SCRATCH, margB, D.mq) SEQ(SCRATCH, margV, D.n * D.n) SEQ(SCRATCH, margW, (D.n + 16) * (D.n + 16))      \
    SEQ(SCRATCH, margE, 3 * D.MX * D.MX + D.n * D.MX) /* marg_exact = 1 only */                                                                 \
    SEQ(STATE, odom, 11) SEQ(STATE, odom_hist, D.hist_cap * 11) SEQ(STATE, odom_count, 1)                                                       \
    DOC("hist_cap (shape key)") DOC("flags")                                                                                                    \
    WIDE("timings", B.timings, 128)                                                                                                             \
    SEQ(SCRATCH, fe_ticks, 4)                                                                                                                   \
    SEQ(STATE, sst, 1) /* idle between frames, but kept: rowbuf and the last solve's diagnostics live here */                                   \
    /* estimate_extrinsic = 2 handles only */                                                                                                   \
    ROW(STATE, "DevCfg::exc", C.exc, D.excal, S * D.excal)                                                                                      \
    ROW(STATE, "DevCfg::exh", C.exh, D.excal * VIO_EXCALIB_CAP * VIO_EXCALIB_PAIR_D, S * D.excal * VIO_EXCALIB_CAP * VIO_EXCALIB_PAIR_D)        \
    /* host vectors of vio_batch: cal / cam mirror the device rows above; the rest travels in the host part of a blob */                        \
    HOST(STATE, "host: last_imu_t", sizeof(double))                                                                                             \
    HOST(STATE, "host: dyn (DynSeq, variable)", 0)                                                                                              \
    HOST(SCRATCH, "host: p_seq p_t p_acc p_gyr (flushed by save, dropped by load)", 0)
enum { ARR_SCRATCH = 0, ARR_STATE = 1, ARR_HANDLE = 2 };   // vio_batch::SnapRow::kind

// allocates every array of the table, zero-filled (B.hist_cap is set before)
inline int handle_alloc_arrays(vio_batch *h) {
    Batch &B = h->B;
    DevCfg &C = h->hc;
    const HandleDims D = handle_dims(C, B.hist_cap);
    const int64_t S = h->S;
    int rc = VIO_OK;
#define VIO_A_SEQ(kind, member, count) if (rc == VIO_OK) rc = dev_alloc(h, &B.member, (size_t)(S * (count)));
#define VIO_A_ROW(kind, name, lvalue, count, n) if (rc == VIO_OK) rc = dev_alloc(h, &lvalue, (size_t)(n));
#define VIO_A_VIEW(kind, name, lvalue, count, at) if (rc == VIO_OK) lvalue = at;
#define VIO_A_WIDE(name, lvalue, n) if (rc == VIO_OK) rc = dev_alloc(h, &lvalue, (size_t)(n));
#define VIO_A_DOC(name)
#define VIO_A_HOST(kind, name, bytes)
    VIO_HANDLE_ARRAYS(VIO_A_SEQ, VIO_A_ROW, VIO_A_VIEW, VIO_A_WIDE, VIO_A_DOC, VIO_A_HOST)
#undef VIO_A_SEQ
#undef VIO_A_ROW
#undef VIO_A_VIEW
#undef VIO_A_WIDE
#undef VIO_A_DOC
#undef VIO_A_HOST
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------- calibration helpers
// the calibration fields of a vio_config (vio_calibration) and back
inline void cal_from_config(const vio_config &c, vio_calibration &k) {
    k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy; k.k1 = c.k1; k.k2 = c.k2; k.p1 = c.p1; k.p2 = c.p2;
    for (int i = 0; i < 9; i++) k.ric[i] = c.ric[i];
    for (int i = 0; i < 3; i++) k.tic[i] = c.tic[i];
    k.td = c.td; k.tr = c.tr;
    k.acc_n = c.acc_n; k.acc_w = c.acc_w; k.gyr_n = c.gyr_n; k.gyr_w = c.gyr_w; k.g_norm = c.g_norm;
}
inline void cal_into_config(const vio_calibration &k, vio_config &c) {
    c.fx = k.fx; c.fy = k.fy; c.cx = k.cx; c.cy = k.cy; c.k1 = k.k1; c.k2 = k.k2; c.p1 = k.p1; c.p2 = k.p2;
    for (int i = 0; i < 9; i++) c.ric[i] = k.ric[i];
    for (int i = 0; i < 3; i++) c.tic[i] = k.tic[i];
    c.td = k.td; c.tr = k.tr;
    c.acc_n = k.acc_n; c.acc_w = k.acc_w; c.gyr_n = k.gyr_n; c.gyr_w = k.gyr_w; c.g_norm = k.g_norm;
}

// the PINHOLE vio_camera of a calibration's fx..p2
inline vio_camera pinhole_camera(const vio_calibration &k) {
    vio_camera m;
    memset(&m, 0, sizeof(m));
    m.model = VIO_CAMERA_PINHOLE;
    const double p[8] = {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2};
    for (int i = 0; i < 8; i++) m.p[i] = p[i];
    return m;
}

// readParameters() re-orthonormalises the extrinsic rotation through a normalised quaternion (parameters.cpp:202-209).  build_devcfg and
// vio_set_calibration share it: a slot and a one-sequence handle of the same calibration then hold the same bits.
inline void ortho_ric(const double *in, double *out) {
    dm::m3 Rc = dm::q2R(dm::qnormalized(dm::R2q(dm::ldm(in))));
    dm::stm(out, Rc);
}

// ---------------------------------------------------------------------------------------------------------------- shared between the files
namespace vio_internal {
// (re)initialise the state of sequences [s_lo, s_hi) (vio_abi.hip)
enum { VIO_RESET_ESTIMATOR = 1, VIO_RESET_TRACKER = 2 };
int init_state(vio_batch *h, int s_lo, int s_hi, int what = VIO_RESET_ESTIMATOR | VIO_RESET_TRACKER);
int flush_imu_backend(vio_batch *h);        // vio_abi.hip
int refresh_dynamic_state(vio_batch *h);    // vio_abi.hip
int launch_marg_all(vio_batch *h);          // vio_abi.hip: what vio_feed launches behind the solve, on every group
// A cut through the solver's launches, for the stage harness only: ps_setup, `slots` whole slots, then the kernels of one more slot up to and
// including phase `stop` (VIO_SOLVE_STOP_*), and no ps_final.  radius0 > 0: SolveSt::radius of every staged sequence is overwritten by a copy between
// ps_setup and the first slot.
struct SolveCut { int slots, stop; double radius0; };
int launch_solve_all(vio_batch *h, const SolveCut *cut);   // vio_abi.hip: the solver launches of vio_feed on every group (nullptr: the whole solve)
// "" when the calibration / camera is usable, else the message naming the offending field (abi_query.hip)
std::string calibration_check(const vio_calibration &k);
std::string camera_check(const vio_camera &m, int width, int height);
}  // namespace vio_internal
