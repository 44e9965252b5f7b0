// Getters and setters of the C ABI (include/vio_abi.h) that do not advance a frame: status, window, odometry, tracks, landmarks, prior,
// calibration, camera, relocalisation, timings, profile, debug, and the device-buffer helpers.  The handle is vio_handle.h.
#include "vio_handle.h"

namespace vio_internal {

// vio_set_calibration's validation: "" when k is usable, else the message naming the offending field (vio_load_seqs applies it to a blob's calibration)
std::string calibration_check(const vio_calibration &k) {
    const struct { const char *name; const double *v; int n; } fin[] = {
        {"fx", &k.fx, 1}, {"fy", &k.fy, 1}, {"cx", &k.cx, 1}, {"cy", &k.cy, 1}, {"k1", &k.k1, 1}, {"k2", &k.k2, 1}, {"p1", &k.p1, 1},
        {"p2", &k.p2, 1}, {"ric", k.ric, 9}, {"tic", k.tic, 3}, {"td", &k.td, 1}, {"tr", &k.tr, 1}, {"acc_n", &k.acc_n, 1},
        {"acc_w", &k.acc_w, 1}, {"gyr_n", &k.gyr_n, 1}, {"gyr_w", &k.gyr_w, 1}, {"g_norm", &k.g_norm, 1}};
    for (const auto &f : fin)
        for (int i = 0; i < f.n; i++)
            if (!std::isfinite(f.v[i])) return std::string(f.name) + " is not finite";
    const struct { const char *name; double v; } pos[] = {
        {"fx", k.fx}, {"fy", k.fy}, {"acc_n", k.acc_n}, {"acc_w", k.acc_w}, {"gyr_n", k.gyr_n}, {"gyr_w", k.gyr_w}, {"g_norm", k.g_norm}};
    for (const auto &f : pos)
        if (!(f.v > 0)) return std::string(f.name) + " must be > 0";
    if (!(k.tr >= 0)) return "tr must be >= 0";
    {
        double err = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double d = (i == j) ? -1.0 : 0.0;
                for (int q = 0; q < 3; q++) d += k.ric[3 * i + q] * k.ric[3 * j + q];
                err = std::max(err, std::fabs(d));
            }
        const double *R = k.ric;
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(err <= 1e-6) || !(det > 0)) return "ric is not a rotation (orthonormal within 1e-6, determinant +1)";
    }
    return "";
}

// vio_set_camera's validation: "" when cam is usable on a width x height image, else the message naming the offending field
std::string camera_check(const vio_camera &m, int width, int height) {
    static const char *const names[3][9] = {{"fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", nullptr},
                                            {"k2", "k3", "k4", "k5", "mu", "mv", "u0", "v0", nullptr},
                                            {"xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0"}};
    if (m.model < VIO_CAMERA_PINHOLE || m.model > VIO_CAMERA_MEI) return "model is not VIO_CAMERA_PINHOLE, _KANNALA_BRANDT or _MEI";
    if (m.reserved != 0) return "reserved must be 0";
    const char *const *nm = names[m.model];
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(m.p[i])) return std::string(i < 9 && nm[i] ? nm[i] : "p[" + std::to_string(i) + "]") + " is not finite";
    const int pos[3][2] = {{0, 1}, {4, 5}, {5, 6}};   // fx fy / mu mv / gamma1 gamma2
    for (int j = 0; j < 2; j++)
        if (!(m.p[pos[m.model][j]] > 0)) return std::string(nm[pos[m.model][j]]) + " must be > 0";
    if (m.model == VIO_CAMERA_MEI && !(m.p[0] >= 0)) return "xi must be >= 0";
    // the four corners and the four edge midpoints must lift in front of the camera: the unit-plane factors hold x / z, y / z
    const double W1 = width - 1, H1 = height - 1;
    const double pts[8][2] = {{0, 0}, {W1, 0}, {0, H1}, {W1, H1}, {W1 / 2, 0}, {W1 / 2, H1}, {0, H1 / 2}, {W1, H1 / 2}};
    for (const auto &q : pts) {
        double x, y, z;
        vcam::lift(m, q[0], q[1], x, y, z);
        if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && z > 0)) {
            char b[160];
            snprintf(b, sizeof(b), "pixel (%g, %g) does not lift to a finite ray in front of the camera (z = %g): the field of view reaches 90 degrees",
                     q[0], q[1], z);
            return b;
        }
    }
    return "";
}

}  // namespace vio_internal
using namespace vio_internal;

extern "C" {

// marg_exact = 2 (the literal marginalisation with a CERTIFIED first inverse): out2 = {marginalisations of sequence seq whose certificate failed
// since vio_create / vio_reset -- those frames used the block inverse WITHOUT the proof that the reference's 1e-8 cut drops nothing --, 1 if the
// last marginalisation was certified}.  A parity run asserts out2[0] == 0; a deployment that sees it grow should switch to marg_exact = 1.
int vio_get_marg_certificate(vio_batch *h, int seq, int32_t *out2) {
    VIO_ENTER(h, seq, false);
    if (!out2) return VIO_EINVAL;
    HIPCHK(hipDeviceSynchronize());
    BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    out2[0] = be.dbg[12]; out2[1] = be.dbg[11];
    return VIO_OK;
}

int vio_get_ex_calibration(vio_batch *h, int seq, double *out16, int cap, double *history) {
    VIO_ENTER(h, seq, false);
    if (!out16 || cap < 0 || (cap > 0 && !history)) return VIO_EINVAL;
    for (int k = 0; k < 16; k++) out16[k] = 0;
    if (!h->hc.exc) return 0;
    HIPCHK(hipDeviceSynchronize());
    ExSeq x;
    BeSeq be;
    HIPCHK(hipMemcpy(&x, h->hc.exc + seq, sizeof(ExSeq), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    out16[0] = be.ex_pending ? 2 : 1;
    out16[1] = x.count;
    out16[2] = x.success_frame;
    for (int k = 0; k < 9; k++) out16[3 + k] = x.ric[k];
    for (int k = 0; k < 4; k++) out16[12 + k] = x.sv[k];
    const int m = std::min(cap, x.count);
    if (m > 0) {
        // the ring holds the newest pairs; hand them out oldest first
        std::vector<double> ring((size_t)VIO_EXCALIB_CAP * VIO_EXCALIB_PAIR_D);
        HIPCHK(hipMemcpy(ring.data(), h->hc.exh + (size_t)seq * VIO_EXCALIB_CAP * VIO_EXCALIB_PAIR_D, ring.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) {
            const double *src = &ring[(size_t)((x.head + i) % VIO_EXCALIB_CAP) * VIO_EXCALIB_PAIR_D];
            for (int k = 0; k < VIO_EXCALIB_PAIR_D; k++) history[(size_t)i * VIO_EXCALIB_PAIR_D + k] = src[k];
        }
    }
    return x.count;
}

int vio_set_relo_frame(vio_batch *h, int seq, double frame_stamp, int frame_index, int n, const double *match_points, const double *relo_t3,
                       const double *relo_r9) {
    VIO_ENTER(h, seq, false);
    if (n < 0 || (n > 0 && !match_points) || !relo_t3 || !relo_r9) return VIO_EINVAL;
    if (n > h->hc.NP) { g_err = "more match points than the tracker holds features (vio_get_capacity)"; return VIO_ECAPACITY; }
    for (int i = 1; i < n; i++)
        if (!(match_points[3 * i + 2] > match_points[3 * (i - 1) + 2])) { g_err = "match points must ascend in feature id"; return VIO_EINVAL; }
    VIO_TRY(sync_all(h));
    h->relo_frames = 1 << 30;   // relocalisation factors use the 42-double records: from now on the two-kernel solver path is launched too (launch_backend)
    double par[15];
    par[0] = frame_stamp; par[1] = frame_index; par[2] = n;
    for (int k = 0; k < 3; k++) par[3 + k] = relo_t3[k];
    for (int k = 0; k < 9; k++) par[6 + k] = relo_r9[k];
    if (n > 0) HIPCHK(hipMemcpy(h->B.relo_mp + (size_t)seq * h->hc.NP * 3, match_points, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_r9, par, sizeof(par), hipMemcpyHostToDevice));
    be_set_relo_kernel<<<1, 64, 0, h->stream>>>(h->B, seq, h->d_r9);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return VIO_OK;
}

int vio_get_relo(vio_batch *h, int seq, double *out30) {
    VIO_ENTER(h, seq, true);
    if (!out30) return VIO_EINVAL;
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    double *o = out30;
    for (int k = 0; k < 3; k++) *o++ = be.relo_relative_t[k];
    for (int k = 0; k < 4; k++) *o++ = be.relo_relative_q[k];
    *o++ = be.relo_relative_yaw;
    for (int k = 0; k < 3; k++) *o++ = be.drift_correct_t[k];
    for (int k = 0; k < 9; k++) *o++ = be.drift_correct_r[k];
    for (int k = 0; k < 7; k++) *o++ = be.relo_Pose[k];
    *o++ = be.relo_info; *o++ = be.relo_local; *o++ = be.relo_factors;
    return VIO_OK;
}

int vio_get_latest_odometry(vio_batch *h, int seq, double *out11) {
    VIO_ENTER(h, seq, false);
    if (!out11) return VIO_EINVAL;
    VIO_TRY(flush_imu_backend(h));   // samples pushed so far must be in the ring
    VIO_TRY(sync_all(h));
    be_latest_odometry_kernel<<<1, 64, 0, h->stream>>>(h->B, seq, h->d_r9);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out11, h->d_r9, 11 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VIO_OK;
}

// staging of the two batched getters below: at least `dev` doubles in HBM and `host` doubles of page-locked memory (nothing of the handle
// is in flight when they are regrown: the callers have synchronised)
static int grow_stage(vio_batch *h, double *&d, size_t &d_cap, double *&hp, size_t &h_cap, size_t dev, size_t host) {
    if (dev > d_cap) {
        dev_release(h, d);
        d_cap = 0;
        VIO_TRY(dev_alloc(h, &d, dev, false));
        d_cap = dev;
    }
    if (host > h_cap) {
        pinned_release(h, hp);
        h_cap = 0;
        VIO_TRY(pinned_alloc(h, &hp, host));
        h_cap = host;
    }
    return VIO_OK;
}
static int odo_stage(vio_batch *h, size_t dev, size_t host) { return grow_stage(h, h->d_odo, h->odo_cap, h->h_odo, h->h_odo_cap, dev, host); }

int vio_get_latest_odometry_all(vio_batch *h, double *out, int on_device) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (!out) return VIO_EINVAL;
    VIO_TRY(flush_imu_backend(h));   // samples pushed so far must be in the ring
    VIO_TRY(sync_all(h));
    const size_t S = (size_t)h->S, o_last = (S + 1) / 2;   // n_rows [S] (int32), then last [S][11]
    VIO_TRY(odo_stage(h, o_last + (on_device ? 0 : S * 11), 0));
    double *last = on_device ? out : h->d_odo + o_last;
    be_imu_rate_odometry_kernel<<<h->S, 64, 0, h->stream>>>(h->B, nullptr, 0, (int *)h->d_odo, nullptr, last);
    HIPCHK(hipGetLastError());
    if (!on_device) HIPCHK(hipMemcpyAsync(out, last, S * 11 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VIO_OK;
}

int vio_get_imu_rate_odometry(vio_batch *h, const double *since, int cap, int32_t *n_rows, double *out, int on_device) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (cap < 0 || !n_rows || (cap > 0 && !out)) return VIO_EINVAL;
    VIO_TRY(flush_imu_backend(h));   // samples pushed so far must be in the ring
    VIO_TRY(sync_all(h));
    // staging, in doubles: since [S], n_rows [S] (int32), rows [S][cap][11] (host output only); the host image holds n_rows and the rows
    const size_t S = (size_t)h->S, o_n = S, o_rows = o_n + (S + 1) / 2, n_row_doubles = on_device ? 0 : S * (size_t)cap * 11;
    VIO_TRY(odo_stage(h, o_rows + n_row_doubles, o_rows + n_row_doubles));
    double *d = h->d_odo, *hb = h->h_odo;
    if (since) {
        memcpy(hb, since, S * sizeof(double));
        HIPCHK(hipMemcpyAsync(d, hb, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    be_imu_rate_odometry_kernel<<<h->S, 64, 0, h->stream>>>(h->B, since ? d : nullptr, cap, (int *)(d + o_n), on_device ? out : d + o_rows, nullptr);
    HIPCHK(hipGetLastError());
    // one copy back: the counts and, for a host output, the rows behind them
    HIPCHK(hipMemcpyAsync(hb + o_n, d + o_n, (o_rows - o_n + n_row_doubles) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t *cnt = (const int32_t *)(hb + o_n);
    for (size_t s = 0; s < S; s++) {
        n_rows[s] = cnt[s];
        const size_t m = (size_t)std::min(cnt[s], cap);
        if (!on_device && m > 0) memcpy(out + s * (size_t)cap * 11, hb + o_rows + s * (size_t)cap * 11, m * 11 * sizeof(double));
    }
    return VIO_OK;
}

int vio_publish_all(vio_batch *h, int cap, int32_t *counts, double *kf_pose, double *cloud, double *margin, double *kf_points, int on_device) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (cap < 0 || !counts) return VIO_EINVAL;
    VIO_TRY(sync_all(h));
    // staging, in doubles: counts [S][4] (int32), kf_pose [S][8], then (host output only) the lists that were asked for, [S][cap][3 | 3 | 8]
    const size_t S = (size_t)h->S, o_pose = 2 * S, o_rows = o_pose + 8 * S, rows = S * (size_t)cap;
    double *const dst[3] = {cloud, margin, kf_points};
    const size_t width[3] = {3, 3, 8};
    size_t off[3], total = o_rows;
    for (int l = 0; l < 3; l++) {
        off[l] = total;
        if (!on_device && dst[l]) total += rows * width[l];
    }
    VIO_TRY(grow_stage(h, h->d_pub, h->pub_cap, h->h_pub, h->h_pub_cap, total, total));
    double *d = h->d_pub, *hb = h->h_pub;
    double *dev[3];
    for (int l = 0; l < 3; l++) dev[l] = !dst[l] ? nullptr : (on_device ? dst[l] : d + off[l]);
    pub_all_kernel<<<h->S, VIO_PUBLISH_BLOCK, 0, h->stream>>>(h->B, cap, (int *)d, on_device ? kf_pose : d + o_pose, dev[0], dev[1], dev[2]);
    HIPCHK(hipGetLastError());
    // one copy back: the counts and, for a host output, the poses and the rows behind them
    HIPCHK(hipMemcpyAsync(hb, d, (on_device ? o_pose : total) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t *cnt = (const int32_t *)hb;
    memcpy(counts, cnt, S * 4 * sizeof(int32_t));
    if (on_device) return VIO_OK;
    for (size_t s = 0; s < S; s++) {
        if (kf_pose && cnt[4 * s + 3]) memcpy(kf_pose + 8 * s, hb + o_pose + 8 * s, 8 * sizeof(double));
        for (int l = 0; l < 3; l++) {
            const size_t m = (size_t)std::min(cnt[4 * s + l], cap);
            if (dst[l] && m > 0) memcpy(dst[l] + s * (size_t)cap * width[l], hb + off[l] + s * (size_t)cap * width[l], m * width[l] * sizeof(double));
        }
    }
    return VIO_OK;
}

int vio_get_packaged(vio_batch *h, int seq, int cap, int32_t *ids, double *obs) {
    VIO_ENTER(h, seq, true);
    static thread_local FeSeq fe;
    HIPCHK(hipMemcpy(&fe, h->B.fe + seq, sizeof(FeSeq), hipMemcpyDeviceToHost));
    if (fe.n_forw < 0 || !fe.publish_ok) return 0;
    int n = fe.n_obs, m = n < cap ? n : cap;
    if (m > 0 && ids) HIPCHK(hipMemcpy(ids, h->B.obs_id + (size_t)seq * h->hc.NP, sizeof(int) * m, hipMemcpyDeviceToHost));
    if (m > 0 && obs) HIPCHK(hipMemcpy(obs, h->B.obs + (size_t)seq * h->hc.NP * 7, sizeof(double) * 7 * m, hipMemcpyDeviceToHost));
    return n;
}

// ---- HBM buffers for callers without their own HIP binding (the on_device = 1 paths take plain device addresses)
void *vio_device_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { g_err = "hipMalloc failed"; return nullptr; }
    return p;
}
void vio_device_free(void *p) { if (p) (void)hipFree(p); }
void *vio_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { g_err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
void vio_host_free(void *p) { if (p) (void)hipHostFree(p); }
int vio_device_upload(void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return VIO_OK; }
int vio_device_download(void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return VIO_OK; }

int vio_get_capacity(vio_batch *h, int32_t *out3) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (!out3) return VIO_EINVAL;
    out3[0] = h->hc.NP; out3[1] = h->hc.NL; out3[2] = h->hc.NIMU;
    return VIO_OK;
}

// which solver the handle runs: 0 = persistent kernel (round-1 fallback), 1 = phased with the Schur complement in LDS tiles, 2 = phased
// with the Schur complement in HBM / L2 (windows beyond W = 10)
int vio_get_solver_kind(vio_batch *h) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    return h->solve_mode == 0 ? 0 : (h->serial_big ? 2 : 1);
}

// bounds-constrained solves of sequence seq since vio_create / vio_reset (estimator.cpp:1282-1297): out4 = inverse depths cut by the bound
// while a point was formed, bounded landmarks that entered solves, trial evaluations and shortened steps of the projected Armijo line search
int vio_get_bound_stats(vio_batch *h, int seq, int64_t *out4) {
    VIO_ENTER(h, seq, false);
    if (!out4) return VIO_EINVAL;
    HIPCHK(hipDeviceSynchronize());
    BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    out4[0] = be.bound_clamps; out4[1] = be.bounded_solves; out4[2] = be.ls_evals; out4[3] = be.ls_contractions;
    return VIO_OK;
}

static void fill_status(const BeSeq &be, const FeSeq &fe, vio_status *out) {
    const int ovf = be.overflow | fe.overflow;
    // a table overflowed in the last frame: results are truncated, say so (bit 512 reports a deviation, not lost capacity)
    out->code = ((ovf & ~VIO_OVF_DEVIATION) && be.status_code == VIO_OK) ? VIO_ECAPACITY : be.status_code;
    out->overflow_flags = ovf; out->overflow_frames = be.overflow_frames;
    out->iterations_total = be.iter_total; out->solves_total = be.solve_total;
    out->solver_flag = be.solver_flag; out->frame_count = be.frame_count;
    out->marginalization_flag = be.marginalization_flag; out->n_landmarks = be.n_lm; out->last_track_num = be.last_track_num;
    out->n_tracks = fe.n_pts; out->processed = be.processed; out->iterations = be.iterations; out->successful_steps = be.successful;
    out->n_in_problem = be.n_in_problem; out->n_residuals = be.n_residuals; out->n_var_landmarks = be.n_var_landmarks;
    out->has_prior = be.has_prior; out->reboot_count = be.reboot_count; out->frames_processed = be.frames_processed;
    out->initial_cost = be.initial_cost; out->final_cost = be.final_cost; out->td = be.td;
}

int vio_get_status(vio_batch *h, int seq, vio_status *out) {
    VIO_ENTER(h, seq, true);
    if (!out) return VIO_EINVAL;
    static thread_local BeSeq be;
    static thread_local FeSeq fe;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&fe, h->B.fe + seq, sizeof(FeSeq), hipMemcpyDeviceToHost));
    fill_status(be, fe, out);
    return VIO_OK;
}

int vio_get_status_all(vio_batch *h, vio_status *out) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!out) return VIO_EINVAL;
    std::vector<BeSeq> be((size_t)h->S);
    std::vector<FeSeq> fe((size_t)h->S);
    HIPCHK(hipMemcpy(be.data(), h->B.be, sizeof(BeSeq) * (size_t)h->S, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fe.data(), h->B.fe, sizeof(FeSeq) * (size_t)h->S, hipMemcpyDeviceToHost));
    for (int s = 0; s < h->S; s++) fill_status(be[s], fe[s], out + s);
    return VIO_OK;
}

int vio_get_window(vio_batch *h, int seq, double *out) {
    VIO_ENTER(h, seq, true);
    if (!out) return VIO_EINVAL;
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    for (int i = 0; i <= h->hc.W; i++) {
        double *o = out + 17 * i;
        dm::quat q = dm::R2q(dm::ldm(be.Rs[i]));
        o[0] = be.Ps[i][0]; o[1] = be.Ps[i][1]; o[2] = be.Ps[i][2];
        o[3] = q.w; o[4] = q.x; o[5] = q.y; o[6] = q.z;
        for (int k = 0; k < 3; k++) { o[7 + k] = be.Vs[i][k]; o[10 + k] = be.Bas[i][k]; o[13 + k] = be.Bgs[i][k]; }
        o[16] = be.Headers[i];
    }
    return VIO_OK;
}

int vio_get_odometry(vio_batch *h, double *out) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!out) return VIO_EINVAL;
    HIPCHK(hipMemcpy(out, h->B.odom, sizeof(double) * (size_t)h->S * 11, hipMemcpyDeviceToHost));
    return VIO_OK;
}

int vio_get_odometry_history(vio_batch *h, int seq, int cap, double *out) {
    VIO_ENTER(h, seq, true);
    if (!out) return VIO_EINVAL;
    int n = 0;
    HIPCHK(hipMemcpy(&n, h->B.odom_count + seq, sizeof(int), hipMemcpyDeviceToHost));
    const int hc = h->B.hist_cap;
    int m = std::min(std::min(n, cap), hc);  // the most recent m rows, oldest first
    const double *base = h->B.odom_hist + (size_t)seq * hc * 11;
    for (int done = 0; done < m;) {
        int row = (n - m + done) % hc, run = std::min(m - done, hc - row);
        HIPCHK(hipMemcpy(out + (size_t)done * 11, base + (size_t)row * 11, sizeof(double) * (size_t)run * 11, hipMemcpyDeviceToHost));
        done += run;
    }
    return n;
}

void vio_calibration_from_config(const vio_config *cfg, vio_calibration *out) {
    if (cfg && out) cal_from_config(*cfg, *out);
}

int vio_set_calibration(vio_batch *h, int seq, const vio_calibration *cal) {
    VIO_ENTER_MSG(h, VIO_NO_SEQ, false, "vio_set_calibration: bad arguments");
    if (!cal) { g_err = "vio_set_calibration: bad arguments"; return VIO_EINVAL; }
    if (seq < 0 || seq >= h->S) { g_err = "vio_set_calibration: seq out of range"; return VIO_EINVAL; }
    const vio_calibration &k = *cal;
    // validation first: the slot is left untouched by a refusal
    const std::string why = calibration_check(k);
    if (!why.empty()) { g_err = "vio_set_calibration: " + why; return VIO_EINVAL; }
    vio_calibration e = k;
    if (h->hc.c.estimate_extrinsic == 2) {   // as build_devcfg: the extrinsic is calibrated online from RIC = I, TIC = 0
        dm::stm(e.ric, dm::eye());
        for (int i = 0; i < 3; i++) e.tic[i] = 0;
    } else {
        ortho_ric(k.ric, e.ric);
    }
    // a fresh slot: synchronise as vio_reset_seq, then the state of a newly created handle for this sequence only
    VIO_TRY(sync_all(h));
    VIO_TRY(refresh_dynamic_state(h));   // a reboot of ANOTHER sequence decided by the last solve must not be lost
    HIPCHK(hipMemcpy(h->d_cal + seq, &e, sizeof(vio_calibration), hipMemcpyHostToDevice));
    h->cal[seq] = e;
    return init_state(h, seq, seq + 1);
}

int vio_get_calibration(vio_batch *h, int seq, vio_calibration *out) {
    VIO_ENTER_MSG(h, seq, false, "vio_get_calibration: bad arguments");
    if (!out) { g_err = "vio_get_calibration: bad arguments"; return VIO_EINVAL; }
    *out = h->cal[seq];
    return VIO_OK;
}

int vio_set_camera(vio_batch *h, int seq, const vio_camera *cam) {
    VIO_ENTER_MSG(h, VIO_NO_SEQ, false, "vio_set_camera: bad arguments");
    if (!cam) { g_err = "vio_set_camera: bad arguments"; return VIO_EINVAL; }
    if (seq < 0 || seq >= h->S) { g_err = "vio_set_camera: seq out of range"; return VIO_EINVAL; }
    // validation first: the slot is left untouched by a refusal
    const std::string why = camera_check(*cam, h->hc.c.width, h->hc.c.height);
    if (!why.empty()) { g_err = "vio_set_camera: " + why; return VIO_EINVAL; }
    vio_camera m = *cam;
    vio_calibration k = h->cal[seq];
    if (m.model == VIO_CAMERA_PINHOLE) {   // the pinhole parameters live in the calibration
        k.fx = m.p[0]; k.fy = m.p[1]; k.cx = m.p[2]; k.cy = m.p[3]; k.k1 = m.p[4]; k.k2 = m.p[5]; k.p1 = m.p[6]; k.p2 = m.p[7];
        m = pinhole_camera(k);
    }
    // a fresh slot, as vio_set_calibration
    VIO_TRY(sync_all(h));
    VIO_TRY(refresh_dynamic_state(h));
    HIPCHK(hipMemcpy(h->d_cal + seq, &k, sizeof(vio_calibration), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_cam + seq, &m, sizeof(vio_camera), hipMemcpyHostToDevice));
    h->cal[seq] = k;
    h->cam[seq] = m;
    return init_state(h, seq, seq + 1);
}

int vio_get_camera(vio_batch *h, int seq, vio_camera *out) {
    VIO_ENTER_MSG(h, seq, false, "vio_get_camera: bad arguments");
    if (!out) { g_err = "vio_get_camera: bad arguments"; return VIO_EINVAL; }
    *out = h->cam[seq].model == VIO_CAMERA_PINHOLE ? pinhole_camera(h->cal[seq]) : h->cam[seq];
    return VIO_OK;
}

int vio_get_extrinsic(vio_batch *h, int seq, double *out13) {
    VIO_ENTER(h, seq, true);
    if (!out13) return VIO_EINVAL;
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) out13[k] = be.tic[k];
    for (int k = 0; k < 9; k++) out13[3 + k] = be.ric[k];
    out13[12] = be.td;
    return VIO_OK;
}

int vio_get_tracks(vio_batch *h, int seq, int cap, int32_t *ids, int32_t *cnt, float *cur, float *un, float *vel) {
    VIO_ENTER(h, seq, true);
    static thread_local FeSeq fe;
    HIPCHK(hipMemcpy(&fe, h->B.fe + seq, sizeof(FeSeq), hipMemcpyDeviceToHost));
    int n = fe.n_pts, m = n < cap ? n : cap;
    size_t o = (size_t)seq * h->hc.NP;
    if (m > 0) {
        HIPCHK(hipMemcpy(ids, h->B.ids + o, sizeof(int) * m, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnt, h->B.track_cnt + o, sizeof(int) * m, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cur, h->B.cur_pts + o, sizeof(float2) * m, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(un, h->B.cur_un_pts + o, sizeof(float2) * m, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(vel, h->B.pts_velocity + o, sizeof(float2) * m, hipMemcpyDeviceToHost));
    }
    return n;
}

static int get_landmarks_impl(vio_batch *h, int seq, int cap, double *out, int width) {
    VIO_ENTER(h, seq, true);
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    const int NL = h->hc.NL, n = be.n_lm, W1 = h->hc.W + 1;
    const size_t o = (size_t)seq * NL;
    // the seven scalar tables are adjacent allocations but not one buffer: one copy each, then (ex only) the observation rows
    std::vector<int> tab((size_t)7 * NL);
    int *order = tab.data(), *id = order + NL, *st = id + NL, *no = st + NL, *ef = no + NL, *sf = ef + NL, *dy = sf + NL;
    std::vector<double> dep(NL);
    HIPCHK(hipMemcpy(order, h->B.lm_order + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(id, h->B.lm_id + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st, h->B.lm_start + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(no, h->B.lm_nobs + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ef, h->B.lm_est_flag + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sf, h->B.lm_solve_flag + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dy, h->B.lm_dyn + o, sizeof(int) * NL, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dep.data(), h->B.lm_depth + o, sizeof(double) * NL, hipMemcpyDeviceToHost));
    std::vector<double> obs;
    if (width > 7) {
        obs.resize((size_t)NL * W1 * VIO_OBS_D);
        HIPCHK(hipMemcpy(obs.data(), h->B.lm_obs + o * W1 * VIO_OBS_D, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < n && k < cap; k++) {
        int s = order[k];
        double *q = out + (size_t)width * k;
        q[0] = id[s]; q[1] = st[s]; q[2] = no[s]; q[3] = dep[s]; q[4] = ef[s]; q[5] = sf[s]; q[6] = dy[s];
        if (width > 7) {
            // feature_per_frame[0] / .back(): the observation rows are ring-indexed per frame (vio_state.h lm_obs)
            const double *f0 = &obs[((size_t)s * W1 + (st[s] + be.ring_base) % W1) * VIO_OBS_D];
            const double *fb = &obs[((size_t)s * W1 + (st[s] + std::max(no[s], 1) - 1 + be.ring_base) % W1) * VIO_OBS_D];
            q[7] = f0[0]; q[8] = f0[1]; q[9] = f0[2]; q[10] = f0[8]; q[11] = fb[8];
        }
    }
    return n;
}
int vio_get_landmarks(vio_batch *h, int seq, int cap, double *out) { return get_landmarks_impl(h, seq, cap, out, 7); }
int vio_get_landmarks_ex(vio_batch *h, int seq, int cap, double *out12) { return get_landmarks_impl(h, seq, cap, out12, 12); }

int vio_get_prior(vio_batch *h, int seq, double *J, double *r, double *x0, uint8_t *present) {
    VIO_ENTER(h, seq, true);
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    if (!be.has_prior) return 0;
    int n = h->hc.NPRIOR, W = h->hc.W;
    if (J || r) {
        // the hot path keeps the prior as a quadratic form (DESIGN.md deviation 13); the factored form the reference stores
        // (linearized_jacobians / linearized_residuals) is produced here, on the GPU, only when somebody asks for it
        be_prior_factor_kernel<<<1, 512, h->lds_factor, h->stream>>>(h->B, seq);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (J) HIPCHK(hipMemcpy(J, h->B.prior_J + (size_t)seq * n * n, sizeof(double) * n * n, hipMemcpyDeviceToHost));
    if (r) HIPCHK(hipMemcpy(r, h->B.prior_rf + (size_t)seq * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (x0) HIPCHK(hipMemcpy(x0, h->B.prior_x0 + (size_t)seq * (W * 7 + 17), sizeof(double) * (W * 7 + 17), hipMemcpyDeviceToHost));
    if (present) for (int k = 0; k < W + 3; k++) present[k] = (uint8_t)be.prior_present[k];
    return n;
}

int vio_get_timings(vio_batch *h, int cap, double *out_ms) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (!out_ms || cap < 3) return VIO_EINVAL;
    if (!h->timing_valid) return 0;
    VIO_TRY(sync_all(h));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    out_ms[0] = a; out_ms[1] = b; out_ms[2] = a + b;
    return 3;
}

int vio_debug_seq(vio_batch *h, int seq, int *out16) {
    VIO_ENTER(h, seq, true);
    static thread_local BeSeq be;
    HIPCHK(hipMemcpy(&be, h->B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; k++) out16[k] = be.dbg[k];
    return VIO_OK;
}

// debug: be_ingest's use of the records of be_preint_ahead_kernel (PreAhead::used / declined), summed and per sequence
int vio_debug_preint_ahead(vio_batch *h, int64_t *out2, int64_t *per_seq) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!out2) return VIO_EINVAL;
    out2[0] = out2[1] = 0;
    if (per_seq) memset(per_seq, 0, (size_t)h->S * 2 * sizeof(int64_t));
    if (!h->d_ahead) return VIO_OK;
    const size_t head = offsetof(PreAhead, pre);   // (the counters precede the pre-integration image)
    std::vector<unsigned char> rec(head);
    for (int s = 0; s < h->S; s++) {
        HIPCHK(hipMemcpy(rec.data(), h->d_ahead + s, head, hipMemcpyDeviceToHost));
        const PreAhead *r = (const PreAhead *)rec.data();
        out2[0] += (int64_t)r->used; out2[1] += (int64_t)r->declined;
        if (per_seq) { per_seq[2 * s] = (int64_t)r->used; per_seq[2 * s + 1] = (int64_t)r->declined; }
    }
    return VIO_OK;
}

// debug: per sequence, the marginalisations that ran as be_marg_pre + be_marg_alg (VIO_MARG_SPLIT; MargSnap::frames); returns their sum in *total
int vio_debug_marg_split(vio_batch *h, int64_t *total, int64_t *per_seq) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!total) return VIO_EINVAL;
    *total = 0;
    if (per_seq) memset(per_seq, 0, (size_t)h->S * sizeof(int64_t));
    if (!h->d_msnap) return VIO_OK;
    for (int s = 0; s < h->S; s++) {
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, (const unsigned char *)(h->d_msnap + s) + offsetof(MargSnap, frames), sizeof(n), hipMemcpyDeviceToHost));
        *total += (int64_t)n;
        if (per_seq) per_seq[s] = (int64_t)n;
    }
    return VIO_OK;
}

// debug: accumulated in-kernel phase ticks (100 MHz) of sequence 0; reset != 0 clears them
int vio_debug_phases(vio_batch *h, float *out128, int reset) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (out128) HIPCHK(hipMemcpy(out128, h->B.timings, 128 * sizeof(float), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(h->B.timings, 0, 128 * sizeof(float)));
    return VIO_OK;
}

// debug: per-sequence in-kernel durations (100 MHz ticks) of the last frame's fe_select / fe_add: out[S][4]
int vio_debug_fe_ticks(vio_batch *h, float *out) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!out) return VIO_EINVAL;
    HIPCHK(hipMemcpy(out, h->B.fe_ticks, (size_t)h->S * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return VIO_OK;
}

// per-kernel HIP-event profile of the next max_steps vio_feed calls (events sit on the batch stream)
int vio_profile_begin(vio_batch *h, int max_steps) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    if (max_steps < 1) return VIO_EINVAL;
    size_t need = (size_t)max_steps * VIO_NEV;
    while (h->pev.size() < need) {
        hipEvent_t e;
        VIO_TRY(new_event(h, &e, hipEventDefault));
        h->pev.push_back(e);
    }
    h->prof_steps = max_steps;
    h->prof_cur = 0;
    h->prof_fe_only = false;
    return VIO_OK;
}
// out_ms[k] = average duration of kernel k over the recorded steps (ms); returns the number of recorded steps
int vio_profile_end(vio_batch *h, int cap, double *out_ms) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (!out_ms || cap < VIO_NK) return VIO_EINVAL;
    int n = h->prof_cur < 0 ? 0 : (h->prof_cur < h->prof_steps ? h->prof_cur : h->prof_steps);
    static const int e0[VIO_NK] = {0, 1, 2, 3, 4, 5, 6, 8, 9, 10}, e1[VIO_NK] = {1, 2, 3, 4, 5, 6, 7, 9, 10, 11};
    for (int k = 0; k < VIO_NK; k++) out_ms[k] = 0;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < (h->prof_fe_only ? 7 : VIO_NK); k++) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, h->pev[(size_t)i * VIO_NEV + e0[k]], h->pev[(size_t)i * VIO_NEV + e1[k]]));
            out_ms[k] += ms;
        }
    for (int k = 0; k < VIO_NK; k++) out_ms[k] = n > 0 ? out_ms[k] / n : 0;
    h->prof_cur = -1;
    return n;
}

}  // extern "C"
