// Kernel entry points shared between the translation units of libvio_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include "vio_state.h"
#include "../../include/vio_synth.h"

// pipelined pre-integration (be_preint.h preint_propagate_many; be_ingest and be_marg run it): samples per chunk, and the LDS doubles
// it borrows from its caller (F 15x15 and V 15x18 of every sample of a chunk); the host sizes the marginalisation's dynamic LDS with the same
// macro
#define PI_CH 8
#define PREINT_MANY_LDS_DOUBLES (PI_CH * (225 + 270))
// dynamic LDS of be_marg.  The overlay region holds, one after the other: the whitened IMU Jacobian, (gj) the packed frame blocks G_j, T1 / A_mr, the
// lower 16x16 tiles of the new prior (Cholesky for its constant term) and the F / V of a chunk of the pre-integration merge in the window slide
__host__ __device__ static inline size_t marg_overlay_bytes(int nprior, int W, bool gj) {
    const size_t nbq = ((size_t)nprior + 15) >> 4, tiles = nbq * (nbq + 1) / 2 * 2048, t1 = (size_t)2 * nprior * 15 * 8, pi = (size_t)PREINT_MANY_LDS_DOUBLES * 8;
    size_t m = tiles > t1 ? tiles : t1;
    m = m > pi ? m : pi;
    if (gj && (size_t)W * 210 * 8 > m) m = (size_t)W * 210 * 8;
    return ((m + 15) & ~(size_t)15) + 64;
}
// be_marg with the reduced system resident in LDS (VIO_MARG_LDS): [overlay | A (15 + n)^2 | b 15 + n | b_r n]; the window slide's landmark tables
// (MARG_LM_TABLES arrays of NL integers) take A's place afterwards
#define MARG_LM_TABLES 6
__host__ __device__ static inline size_t marg_resident_doubles(int nprior) { const size_t q = (size_t)nprior + 15; return q * q + q + (size_t)nprior; }
__host__ __device__ static inline size_t marg_resident_lds_bytes(int nprior, int W) { return marg_overlay_bytes(nprior, W, true) + marg_resident_doubles(nprior) * 8; }
// dynamic LDS of fast_cell (fe_kernels.hip) for a rw x rh region: tile (pitch up to rw + 6) + score plane + NMS ballot words
static inline size_t fast_lds_bytes(int rw, int rh) {
    return (size_t)(((rw + 6) * rh + 15) & ~15) + (size_t)((rw * rh + 15) & ~15) + (size_t)(((rw - 6) * (rh - 6) + 63) / 64 + 2) * 8 + 16;
}
// dynamic LDS of one evaluation role of ps_eval (be_phased.h): frame-pair geometry / staged pre-integration headers
__host__ __device__ static inline size_t ps_eval_lds_bytes(int W) {
    const size_t W1 = (size_t)W + 1, a = (W1 * W1 + 1) * 32 * 8, b = (size_t)W * (VIO_PREINT_HDR + 1) * 8;
    return (a > b ? a : b) + 64;
}
// dynamic LDS of ps_ls_kernel: evaluation point + scalar workspace + partial costs (PS_LS_HEAD_DOUBLES); the evaluation roles' region is in HBM (Batch::ls_scratch)
static inline size_t ps_ls_lds_bytes(int W) { (void)W; return ((((sizeof(Params) / sizeof(double)) + 1) & ~(size_t)1) + 176) * 8 + 16; }
struct LkImages {
    const uint8_t *prev[4];
    const uint8_t *next[4];
    int w[4], h[4];
};

__global__ void fe_begin_kernel(Batch B, const double *stamps, int gate, int publish, const uint8_t *modes, const double *R_rel);
__global__ void be_latest_odometry_kernel(Batch B, int seq, double *out11);
__global__ void be_imu_rate_odometry_kernel(Batch B, const double *since, int cap, int *n_rows, double *rows, double *last);
// pubPointCloud / pubKeyframe for the whole batch (pub_kernels.hip): one sequence's tables as plain pointers, and where its four outputs go.
// pub_all_kernel fills a PubIn per sequence from the Batch, pub_stage_kernel takes one from the host (vio_stage_publish).
struct PubIn {
    const int *lm_order, *lm_id, *lm_start, *lm_nobs, *lm_solve_flag, *lm_dyn;   // [NL]; lm_order lists the live slots in list order
    const double *lm_depth;      // [NL] estimated_depth
    const double *lm_obs;        // [NL][W+1][VIO_OBS_D], ring-indexed per frame
    int n_lm, NL, W, ring_base;
    const double *Ps, *Rs, *Headers, *ric, *tic;   // [W+1][3], [W+1][9] row-major, [W+1], [9], [3]
    int solver_flag, marginalization_flag, processed;
};
struct PubOut {
    int cap;             // rows of cloud / margin / kf_points; nothing is written at or beyond it
    int *counts;         // [4] n_cloud n_margin n_kf kf_valid
    double *kf_pose;     // [8] stamp P(3) Q(w, x, y, z) of window frame W - 2, written only when kf_valid
    double *cloud, *margin, *kf_points;   // [cap][3], [cap][3], [cap][8], or NULL: counted only
};
__global__ void pub_all_kernel(Batch B, int cap, int *counts, double *kf_pose, double *cloud, double *margin, double *kf_points);
__global__ void pub_stage_kernel(PubIn in, PubOut out);
__global__ void fe_predict_motion_kernel(Batch B, int seq, double t0, double t1, double *out9);
__global__ void fe_pyrdown_kernel(Batch B, const uint8_t *src_base, size_t src_stride, int sw, int sh, int dst_level, int write_level0);
__global__ void fe_pyrdown_stage_kernel(const uint8_t *src, int sw, int sh, uint8_t *dst);
__global__ void fe_clahe_lut_kernel(Batch B, const uint8_t *src_base, size_t stride);
__global__ void fe_clahe_apply_kernel(Batch B, const uint8_t *src_base, size_t stride);
__global__ void fe_clahe_lut_stage_kernel(const uint8_t *src, int W, int H, uint8_t *lut);
__global__ void fe_clahe_apply_stage_kernel(const uint8_t *src, int W, int H, const uint8_t *lut, uint8_t *dst);
__global__ void fe_predict_kernel(Batch B);
__global__ void fe_lk_kernel(Batch B);
__global__ void fe_lk_stage_kernel(LkImages im, int maxLevel, int n, const float2 *prevPts, float2 *nextPts, uint8_t *status);
__global__ void fe_ransac_stage_kernel(vio_config c, int n, const float2 *p1, const float2 *p2, uint8_t *status);
// vio_stage_camera: camera_model.h through the tracker's device code (lift, x / z and y / z, spaceToPlane(R * ray)); R9 = 9 doubles
__global__ void fe_camera_stage_kernel(vio_camera cam, int n, const double *uv, const double *R9, double *ray, double *un, double *uv_out);
__global__ void fe_select_kernel(Batch B);
__global__ void fe_fast_kernel(Batch B);
__global__ void fe_fast_stage_kernel(const uint8_t *img, int W, GridRect r, uint32_t *out, int cap, int *count);
__global__ void fe_add_kernel(Batch B, int gate);
struct PreAhead;
// feature-map source of be_ingest: ids == NULL selects the map packaged on the device by the front-end
struct IngestSrc {
    const int *n_obs;       // [S] entries per sequence (< 0: skip the sequence)
    const int *ids;         // [S][cap] ascending feature ids
    const double *obs;      // [S][cap][7] x y z u v vx vy
    const double *stamps;   // [S] header stamps
    int cap;
    PreAhead *ahead;        // [S] (indexed by sequence) results of be_preint_ahead_kernel for this frame, or NULL: be_ingest integrates the IMU itself
};
// One sequence's record of be_preint_ahead_kernel: the frame's IMU interval pre-integrated, and processIMU's world-state step taken, beside be_marg of
// the previous frame.  A per-call buffer of the handle (vio_batch::d_ahead), not per-sequence state: it is in no table and in no snapshot.  be_ingest takes
// the result over only where every input recorded here has, bit for bit, the value it would use itself; otherwise it integrates as ever.
//   in      acc_0 gyr_0 Ps[W] Vs[W] Rs[W] Bas[W] Bgs[W] g   (acc_0 / gyr_0 / Bas[W] / Bgs[W] are also the fresh slot's lin_acc / lin_gyr / lin_ba / lin_bg)
//   noise   acc_n gyr_n acc_w gyr_w of the sequence's calibration
//   out     Ps[W] Vs[W] Rs[W] acc_0 gyr_0 after the interval
//   pre     the pre-integration of slot W: everything up to the sample buffers, and the first min(n, VIO_IMU_SLOT_CAP) entries of those
struct PreAhead {
    double stamp, cur_time, prev_time;
    double in[30], noise[4];
    int imu_head, imu_count;   // BeSeq::imu_head / imu_count the interval search started from
    int valid;                 // 0: nothing was computed (not steady state, ring overrun, the IMU does not reach cur_time yet)
    int head, k, n;            // first sample of the interval, the first one at or after cur_time, their number (k - head + 1)
    double out[21];
    unsigned long long used, declined;   // frames of this sequence for which be_ingest took the record over / integrated itself although it was handed one
    PreInt pre;
};
static_assert(offsetof(PreInt, dt_buf) == (VIO_PREINT_HDR + 225) * sizeof(double), "PreInt: what be_ingest takes over from a PreAhead whole");
// S workgroups x 256 threads, on the front-end stream once the previous frame's solve has ended (its ev_solve); stamps: the call's [S] header stamps
__global__ void be_preint_ahead_kernel(Batch B, const double *stamps, PreAhead *ahead);
template <bool EXCALIB> __global__ void be_ingest_kernel(Batch B, const uint16_t *depth_base, size_t depth_stride, IngestSrc src);
__global__ void be_stage_relative_r_kernel(int n, const double *corres6, double *R9, int *detail8);
__global__ void be_solve_kernel(Batch B);
__global__ void be_solve_kernel_512(Batch B);
__global__ void be_marg_kernel(Batch B);       // reduced system, frame blocks and landmark tables in LDS (vio_batch::marg_lds)
__global__ void be_marg_hbm_kernel(Batch B);   // the same stage with them in HBM scratch: windows whose system does not fit, VIO_MARG_LDS = 0
__global__ void be_marg_exact_kernel(Batch B);
// VIO_MARG_SPLIT: be_marg_kernel cut along its phase boundary, so that the next frame's be_ingest and ps_setup can run beside the algebra.
//   be_marg_pre_kernel  everything that reads or writes window state shared with the next frame: the marginalisation's vector2double, the list of the
//                       landmarks that start in frame 0 and their projection records (into Batch::res), then the window slide (finish_body)
//   be_marg_alg_kernel  the algebra, from what the first one left in a MargSnap, the list, the records and the OLD prior: prior part, IMU factor, landmark
//                       rows, frame blocks, rank update, elimination of the m-block, the new prior.  It reads nothing finish_body, be_ingest or ps_setup
//                       write and writes nothing those two read.
// Same device code (marg_body), same operands in the same order: the pair leaves the bits be_marg_kernel leaves.
// One sequence's hand-over record.  Like PreAhead a per-call buffer of the handle (vio_batch::d_msnap), dead once be_marg_alg has run: in no table, in
// no snapshot.  The list (mlist: [S][2][NL] integers, vio_batch::d_mlist) holds the slots of the landmarks that start in frame 0, then each entry's
// observation count as it was before the slide.
struct MargSnap {
    Params X;                   // the window as the solve left it (relo is not carried)
    double g[3];
    int active;                 // this frame marginalises (be_marg_kernel's guards, taken before the slide)
    int second_new;             // marginalization_flag != 0
    int pre1;                   // pre_idx[1] before the slide: the pre-integration between frames 0 and 1
    int F0c;                    // landmarks in the list (0 for MARGIN_SECOND_NEW)
    unsigned long long frames;  // marginalisations of this sequence that took the split path (vio_debug_marg_split)
};
__global__ void be_marg_pre_kernel(Batch B, MargSnap *snap, int *mlist);
__global__ void be_marg_alg_kernel(Batch B, MargSnap *snap, const int *mlist);
// dynamic LDS of be_marg_exact_kernel's LDS-resident eigen-decomposition of an m x m block (be_kernels.hip marg_exact_finish / marg_literal_prior)
static inline size_t marg_exact_lds_bytes(int m) { return ((size_t)m * (m | 1) + 11 * (size_t)(6 * VIO_MAXW + 16)) * 8 + 64; }
// ... and of the blocks that do not fit: sym_eig_hbm's vectors (be_linalg.h SYM_EIG_HBM_LDS_DOUBLES; be_kernels.hip asserts the two agree)
#define MARG_EXACT_HBM_LDS_DOUBLES (7 * 512)
static inline size_t marg_exact_hbm_lds_bytes() { return (size_t)MARG_EXACT_HBM_LDS_DOUBLES * 8 + 64; }
// vio_stage_marg_literal: one part of the literal marginalisation (be_kernels.hip) on caller-supplied data, one workgroup.  Every array is a
// segment of one scratch allocation of the host side (abi_stage.hip), which puts guard words between them; the kernel fills a Ctx from them.
//   part 0  marg_exact_finish:   A (mq x mq, mq = md + n), b (mq), Cl (F0 x ldc), Hll = d (F0), gl (F0) -> margE (A_mm^+, A_rm A_mm^+), margV = A_r,
//                                vec = b_r, the prior
//   part 1  marg_literal_prior:  margV = A_r (n x n), vec = b_r -> prior_J, prior_rf, prior_H, prior_r, BeSeq::prior_c0
//   part 2  marg_certificate:    A = Pinv (md x md), Cl, Hll = 1 / d or 0 -> info[0] = certified, scal[1] = the bound
struct MargLiteralStage {
    const DevCfg *cfg;   // MX, MXL
    BeSeq *be;
    double *A, *b, *Cl, *Hll, *gl;
    double *margE, *margV, *margW, *vec, *prior_J, *prior_H, *prior_r, *prior_rf;
    double *scal;        // [0] BeSeq::prior_c0, [1] the certificate's bound
    int *info;           // [0] certified, [1 ..] BeSeq::dbg[0], [2], [4]
    int part, md, F0, n, ldc, pinv_direct, second_new;
};
__global__ void be_stage_marg_literal_kernel(MargLiteralStage a);
// phased solver (be_phased.h)
__global__ void ps_setup_kernel(Batch B);
__global__ void ps_eval_kernel(Batch B);
__global__ void ps_asm_a_kernel(Batch B);
__global__ void ps_asm_b_schur_kernel(Batch B, int nb_b);
__global__ void ps_serial_big_kernel(Batch B);
__global__ void ps_serial_kernel_512(Batch B);
__global__ void ps_final_kernel(Batch B);
__global__ void ps_ls_kernel(Batch B);
__global__ void ps_evalf_kernel(Batch B);
// dynamic LDS of ps_evalf_kernel: a chunk's records + the frame-pair geometry (by pair slot), (+ the chunk's landmark table), or (workgroup 1) staged pre-integration headers + raw IMU
// Jacobians, or (workgroup 0) the prior's vectors
static inline size_t ps_evalf_lds_bytes(int W) {
    const size_t W1 = (size_t)W + 1, a = ((size_t)PS_FUSE_CAP * 28 + (W1 * W / 2 + 1) * 32) * 8 + (size_t)PS_FUSE_CAP * 12, b = ((size_t)W * (VIO_PREINT_HDR + 1) + (size_t)W * 465) * 8;
    return (a > b ? a : b) + 16;
}
__global__ void be_prior_factor_kernel(Batch B, int seq);
__global__ void be_set_relo_kernel(Batch B, int seq, const double *par);
__global__ void be_stage_pnp_kernel(const double *pts, int n, double *par6, int *trace4);
__global__ void be_stage_rodrigues_kernel(int mode, int n, const double *in, double *out);
__global__ void be_dyn_finalize_kernel(Batch B, int seq, const double *samples, const int *offs);
__global__ void be_stage_imu_kernel(vio_config cfg, PreInt *P, int n, const double *dt, const double *acc, const double *gyr,
                                    const double *par, double g_norm, double *preint_out, double *r15, double *J480);
__global__ void be_stage_projection_kernel(vio_config cfg, const double *in, int use_td, int form, double *r2, double *J46);
__global__ void be_stage_imu_block_kernel(const PreInt *P, const double *par, double g_norm, double *G961);
__global__ void be_stage_preint_kernel(vio_config cfg, PreInt *P, int n, const double *dt, const double *acc, const double *gyr, int mode,
                                       double *out686);
// Sample source of preint_propagate_many (be_preint.h) in be_ingest and in its stage harness: the frame's interval of a sequence's IMU
// ring (getIMUInterval + the dt of processMeasurements, estimator.cpp:185-200): n samples from `head`, the last one being the first at or
// after curTime.  dt runs from prevTime to the first stamp, between stamps, and up to curTime.
struct PreintRing {
    const double *it, *ia, *ig; int head, NIMU; double prevTime, curTime; int n;
    __device__ __forceinline__ void get(int q, double &dt_q, double *acc_q, double *gyr_q) const {
        const int idx = (head + q) % NIMU;
        const double tq = it[idx];
        if (q == 0) dt_q = tq - prevTime;
        else if (q == n - 1) dt_q = curTime - it[(head + q - 1) % NIMU];
        else dt_q = tq - it[(head + q - 1) % NIMU];
        for (int k = 0; k < 3; k++) { acc_q[k] = ia[(size_t)idx * 3 + k]; gyr_q[k] = ig[(size_t)idx * 3 + k]; }
    }
};
__global__ void be_stage_preint_ring_kernel(vio_config cfg, PreInt *P, PreintRing ring, double *world31, double *out686);
__global__ void be_stage_imu_raw_kernel(const PreInt *P, const double *par, double g_norm, double *r15, double *J450, double *Jp465);
__global__ void be_stage_projection_pair_kernel(vio_config cfg, const double *in, int use_td, int cauchy, int rs, int ext, double *r2, double *wgt,
                                                double *J);
__global__ void be_stage_pose_ops_kernel(int n, const double *x7, const double *d6, const double *x07, double *plus7, double *dx6);
__global__ void imu_scatter_kernel(Batch B, int total, const int *seq_of, const double *t, const double *acc, const double *gyr);
__global__ void imu_commit_kernel(Batch B, int total, const int *seq_of);
__global__ void synth_render_kernel(vio_synth_config c, int S, uint64_t seq0, const float *rays, const float *poses, uint8_t *gray, uint16_t *depth);
