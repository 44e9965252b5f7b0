// The publishers that read the landmark table, for every sequence in one launch: pubPointCloud's cloud and margin cloud
// (visualization.cpp:328-407) and pubKeyframe's pose and 2D-3D points (visualization.cpp:454-520).  One device routine (publish_seq) on
// plain pointers for one sequence; pub_all_kernel hands it a sequence of a Batch, pub_stage_kernel caller-supplied tables
// (vio_stage_publish).  Output only: nothing the estimator reads is written.
#include "kernels.h"
#include "dmath.h"

namespace {

// w_pts_i = Rs[imu_i] * (ric * pts_i + tic) + Ps[imu_i] (visualization.cpp:346-355, :388-396, :489-498) with
// pts_i = feature_per_frame[0].point * (depth == 0 ? estimated_depth : depth), in the operation order of Estimator::pointCloud()
// (include/vio_adapter.hpp): each row is ((a + b) + c) + offset
__device__ __forceinline__ dm::v3 world_point(const PubIn &in, int start, const double *obs0, double est_depth) {
    const double d = obs0[8] == 0 ? est_depth : obs0[8];
    const dm::v3 pc = dm::mk(obs0[0] * d, obs0[1] * d, obs0[2] * d);
    const dm::v3 pi = dm::add(dm::mul(dm::ldm(in.ric), pc), dm::ld3(in.tic));
    return dm::add(dm::mul(dm::ldm(in.Rs + 9 * start), pi), dm::ld3(in.Ps + 3 * start));
}

// One workgroup of VIO_PUBLISH_BLOCK threads, one sequence.  The list lm_order[0 .. n_lm) is walked in list order (the iteration order of
// f_manager.feature) in chunks of the block size; every output list is compacted with a ballot per wavefront and the wavefront totals in
// LDS, a running base is carried from chunk to chunk, so the rows come out in list order whatever the scheduling.  Rows at and beyond
// `cap` are counted and not written; a NULL list is counted only.
__device__ void publish_seq(const PubIn &in, const PubOut &out) {
    constexpr int NWAVE = VIO_PUBLISH_BLOCK / 64;
    __shared__ int wave_total[3][NWAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = in.W, W1 = W + 1, NL = in.NL;
    const int n = in.n_lm < 0 ? 0 : (in.n_lm > NL ? NL : in.n_lm);
    const int ring = ((in.ring_base % W1) + W1) % W1;
    // pubKeyframe's guard (visualization.cpp:457-458); the nodelet calls the publishers for processed frames only
    const bool kf_valid = in.solver_flag == 1 && in.marginalization_flag == 0 && in.processed != 0 && W >= 2;
    int base[3] = {0, 0, 0};
    for (int k0 = 0; k0 < n; k0 += VIO_PUBLISH_BLOCK) {
        const int k = k0 + tid;
        bool want[3] = {false, false, false};
        int slot = -1, start = 0;
        if (k < n) {
            slot = in.lm_order[k];
            if (slot >= 0 && slot < NL) {
                start = in.lm_start[slot];
                const int n_obs = in.lm_nobs[slot];
                const bool solved = in.lm_solve_flag[slot] == 1, dyn = in.lm_dyn[slot] != 0;
                if (start >= 0 && start <= W) {   // (a start outside the window indexes no pose)
                    // visualization.cpp:335-344
                    const bool used = !dyn && n_obs >= 2 && start < W - 2;
                    want[0] = used && !(start > W * 3.0 / 4.0) && solved;
                    // visualization.cpp:373-386
                    want[1] = used && start == 0 && n_obs <= 2 && solved;
                    // visualization.cpp:484-487 (no is_dynamic test there)
                    want[2] = kf_valid && start < W - 2 && start + n_obs - 1 >= W - 2 && solved;
                }
            }
        }
        int row[3];
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const unsigned long long bal = __ballot(want[l]);
            row[l] = __popcll(bal & ((1ULL << lane) - 1ULL));
            if (lane == 0) wave_total[l][wave] = __popcll(bal);
        }
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 3; l++) {
            int before = 0, total = 0;
            for (int w = 0; w < NWAVE; w++) {
                const int t = wave_total[l][w];
                if (w < wave) before += t;
                total += t;
            }
            row[l] += base[l] + before;
            base[l] += total;
        }
        __syncthreads();
        if (want[0] || want[1] || want[2]) {
            // feature_per_frame[0]: the row of window frame `start`, addressed as obs_ptr (be_ctx.h): physical = (frame + ring_base) % (W + 1)
            const double *obs0 = in.lm_obs + ((size_t)slot * W1 + (start + ring) % W1) * VIO_OBS_D;
            const dm::v3 pw = world_point(in, start, obs0, in.lm_depth[slot]);
            if (want[0] && out.cloud && row[0] < out.cap) dm::st3(out.cloud + (size_t)row[0] * 3, pw);
            if (want[1] && out.margin && row[1] < out.cap) dm::st3(out.margin + (size_t)row[1] * 3, pw);
            if (want[2] && out.kf_points && row[2] < out.cap) {
                // feature_per_frame[WINDOW_SIZE - 2 - start_frame] = the row of window frame W - 2 (visualization.cpp:505-511)
                const double *oj = in.lm_obs + ((size_t)slot * W1 + (W - 2 + ring) % W1) * VIO_OBS_D;
                double *o = out.kf_points + (size_t)row[2] * 8;
                dm::st3(o, pw);
                o[3] = oj[0]; o[4] = oj[1]; o[5] = oj[3]; o[6] = oj[4];
                o[7] = (double)in.lm_id[slot];
            }
        }
    }
    if (tid == 0) {
        out.counts[0] = base[0]; out.counts[1] = base[1]; out.counts[2] = kf_valid ? base[2] : 0; out.counts[3] = kf_valid ? 1 : 0;
        if (kf_valid && out.kf_pose) {
            // visualization.cpp:460-474; the matrix -> quaternion routine of vio_get_window
            const dm::quat q = dm::R2q(dm::ldm(in.Rs + 9 * (W - 2)));
            double *o = out.kf_pose;
            o[0] = in.Headers[W - 2];
            o[1] = in.Ps[3 * (W - 2)]; o[2] = in.Ps[3 * (W - 2) + 1]; o[3] = in.Ps[3 * (W - 2) + 2];
            o[4] = q.w; o[5] = q.x; o[6] = q.y; o[7] = q.z;
        }
    }
}

}  // namespace

// grid S, VIO_PUBLISH_BLOCK threads.  counts [S][4], kf_pose [S][8], cloud / margin [S][cap][3] or NULL, kf_points [S][cap][8] or NULL
__global__ __launch_bounds__(VIO_PUBLISH_BLOCK) void pub_all_kernel(Batch B, int cap, int *counts, double *kf_pose, double *cloud, double *margin,
                                                                     double *kf_points) {
    const int s = blockIdx.x;
    if (s >= B.S) return;
    const BeSeq &be = B.be[s];
    const size_t o = (size_t)s * B.gNL;
    PubIn in;
    in.lm_order = B.lm_order + o; in.lm_id = B.lm_id + o; in.lm_start = B.lm_start + o; in.lm_nobs = B.lm_nobs + o;
    in.lm_solve_flag = B.lm_solve_flag + o; in.lm_dyn = B.lm_dyn + o; in.lm_depth = B.lm_depth + o;
    in.lm_obs = B.lm_obs + o * (B.gW + 1) * VIO_OBS_D;
    in.n_lm = be.n_lm; in.NL = B.gNL; in.W = B.gW; in.ring_base = be.ring_base;
    in.Ps = &be.Ps[0][0]; in.Rs = &be.Rs[0][0]; in.Headers = be.Headers; in.ric = be.ric; in.tic = be.tic;
    in.solver_flag = be.solver_flag; in.marginalization_flag = be.marginalization_flag; in.processed = be.processed;
    PubOut out;
    const size_t r = (size_t)s * (size_t)cap;
    out.cap = cap; out.counts = counts + 4 * s; out.kf_pose = kf_pose ? kf_pose + 8 * s : nullptr;
    out.cloud = cloud ? cloud + r * 3 : nullptr; out.margin = margin ? margin + r * 3 : nullptr;
    out.kf_points = kf_points ? kf_points + r * 8 : nullptr;
    publish_seq(in, out);
}

// vio_stage_publish: the same routine on one synthetic sequence
__global__ __launch_bounds__(VIO_PUBLISH_BLOCK) void pub_stage_kernel(PubIn in, PubOut out) {
    if (blockIdx.x != 0) return;
    publish_seq(in, out);
}
