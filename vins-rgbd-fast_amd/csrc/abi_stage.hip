// Stage entry points of the C ABI (include/vio_abi.h vio_stage_*): one front-end or back-end building block on caller-supplied data, for the
// parity tests.  No handle: every call allocates what it needs for its own duration (DevBuf, stage_util.h).
#include "vio_handle.h"

extern "C" {

int vio_stage_host_camera(const vio_camera *cam, int n, const double *uv, const double *R9, double *ray_out, double *un_out, double *uv_out) {
    if (!cam || n < 0 || (n > 0 && !uv)) return VIO_EINVAL;
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double *R = R9 ? R9 : I9;
    for (int i = 0; i < n; i++) {
        double x, y, z, X, Y, Z;
        vcam::lift(*cam, uv[2 * i], uv[2 * i + 1], x, y, z);
        if (ray_out) { ray_out[3 * i] = x; ray_out[3 * i + 1] = y; ray_out[3 * i + 2] = z; }
        if (un_out) vcam::lift_plane(*cam, uv[2 * i], uv[2 * i + 1], un_out[2 * i], un_out[2 * i + 1]);
        X = R[0] * x + R[1] * y + R[2] * z; Y = R[3] * x + R[4] * y + R[5] * z; Z = R[6] * x + R[7] * y + R[8] * z;
        if (uv_out) vcam::project(*cam, X, Y, Z, uv_out[2 * i], uv_out[2 * i + 1]);
    }
    return VIO_OK;
}

int vio_stage_pyr_down(const uint8_t *src, int w, int h, uint8_t *dst) {
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    DevBuf<uint8_t> ds, dd;
    HIPCHK(ds.alloc((size_t)w * h));
    HIPCHK(dd.alloc((size_t)dw * dh));
    HIPCHK(ds.upload(src, (size_t)w * h));
    fe_pyrdown_stage_kernel<<<dim3((dw + 63) / 64, (dh + 15) / 16), 256>>>(ds, w, h, dd);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dd.download(dst, (size_t)dw * dh));
    return VIO_OK;
}

int vio_stage_clahe(const uint8_t *src, int w, int h, uint8_t *dst) {
    DevBuf<uint8_t> ds, dd, dl;
    if (!src || !dst || w < 8 || h < 8) return VIO_EINVAL;
    HIPCHK(ds.alloc((size_t)w * h));
    HIPCHK(dd.alloc((size_t)w * h));
    HIPCHK(dl.alloc(64 * 256));
    HIPCHK(ds.upload(src, (size_t)w * h));
    fe_clahe_lut_stage_kernel<<<64, 256>>>(ds, w, h, dl);
    fe_clahe_apply_stage_kernel<<<dim3((w + 1023) / 1024, h), 256>>>(ds, w, h, dl, dd);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dd.download(dst, (size_t)w * h));
    return VIO_OK;
}

int vio_stage_fast_roi(const uint8_t *img, int W, int H, int rx, int ry, int rw, int rh, int cap, float *out) {
    int count = 0;
    DevBuf<uint8_t> di;
    DevBuf<uint32_t> dout;
    DevBuf<int> dcnt;
    std::vector<uint32_t> hv;
    GridRect r{rx, ry, rw, rh};
    if (rw < 7 || rh < 7) return 0;
    size_t lds = fast_lds_bytes(rw, rh);
    HIPCHK(di.alloc((size_t)W * H));
    HIPCHK(dout.alloc((size_t)cap));
    HIPCHK(dcnt.alloc(1));
    HIPCHK(di.upload(img, (size_t)W * H));
    (void)raise_lds_limit((const void *)fe_fast_stage_kernel, (size_t)(lds));
    fe_fast_stage_kernel<<<1, 256, lds>>>(di, W, r, dout, cap, dcnt);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dcnt.download(&count, 1));
    hv.resize(cap);
    HIPCHK(dout.download(hv.data(), (size_t)cap));
    for (int i = 0; i < count && i < cap; i++) { out[3 * i] = (float)(hv[i] & 0xFFF); out[3 * i + 1] = (float)((hv[i] >> 12) & 0xFFF); out[3 * i + 2] = (float)(hv[i] >> 24); }
    return count;
}

int vio_stage_lk(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, int n, const float *prev_pts, float *next_pts,
                 uint8_t *status) {
    if (max_level < 0 || max_level > 3 || n < 0) return VIO_EINVAL;
    max_level = vio_lk_effective_level(w, h, max_level);
    DevBuf<uint8_t> dp[4], dn[4], dst;
    DevBuf<float2> dpp, dnp;
    LkImages im;
    memset(&im, 0, sizeof(im));
    int lw = w, lh = h;
    for (int l = 0; l <= max_level; l++) {
        HIPCHK(dp[l].alloc((size_t)lw * lh));
        HIPCHK(dn[l].alloc((size_t)lw * lh));
        im.prev[l] = dp[l]; im.next[l] = dn[l]; im.w[l] = lw; im.h[l] = lh;
        if (l == 0) {
            HIPCHK(dp[0].upload(prev, (size_t)w * h));
            HIPCHK(dn[0].upload(next, (size_t)w * h));
        } else {
            int pw = im.w[l - 1], ph = im.h[l - 1];
            fe_pyrdown_stage_kernel<<<dim3((lw + 63) / 64, (lh + 15) / 16), 256>>>(dp[l - 1], pw, ph, dp[l]);
            fe_pyrdown_stage_kernel<<<dim3((lw + 63) / 64, (lh + 15) / 16), 256>>>(dn[l - 1], pw, ph, dn[l]);
        }
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
    }
    HIPCHK(dpp.alloc((size_t)n + 1));
    HIPCHK(dnp.alloc((size_t)n + 1));
    HIPCHK(dst.alloc((size_t)n + 1));
    HIPCHK(dpp.upload((const float2 *)prev_pts, n));
    HIPCHK(dnp.upload((const float2 *)next_pts, n));
    if (n > 0) fe_lk_stage_kernel<<<n, 64>>>(im, max_level, n, dpp, dnp, dst);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dnp.download((float2 *)next_pts, n));
    HIPCHK(dst.download(status, n));
    return VIO_OK;
}

int vio_stage_ransac(const vio_config *cfg, int n, const float *p1, const float *p2, uint8_t *status) {
    DevBuf<float2> d1, d2;
    DevBuf<uint8_t> ds;
    size_t lds = (size_t)n * 36 + 64;
    HIPCHK(d1.alloc((size_t)n + 1));
    HIPCHK(d2.alloc((size_t)n + 1));
    HIPCHK(ds.alloc((size_t)n + 1));
    HIPCHK(d1.upload((const float2 *)p1, n));
    HIPCHK(d2.upload((const float2 *)p2, n));
    (void)raise_lds_limit((const void *)fe_ransac_stage_kernel, (size_t)(lds));
    fe_ransac_stage_kernel<<<1, 256, lds>>>(*cfg, n, d1, d2, ds);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(ds.download(status, n));
    return VIO_OK;
}

int vio_stage_camera(const vio_camera *cam, int n, const double *uv, const double *R9, double *ray_out, double *un_out, double *uv_out) {
    if (!cam || n < 0 || (n > 0 && !uv)) return VIO_EINVAL;
    DevBuf<double> d;
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const size_t m = (size_t)n + 1;   // uv(2) ray(3) un(2) uv_out(2) per point, R9
    HIPCHK(d.alloc(9 * m + 9));
    HIPCHK(d.upload(uv, (size_t)2 * n));
    HIPCHK(d.upload(R9 ? R9 : I9, 9, 9 * m));
    if (n > 0) fe_camera_stage_kernel<<<(n + 255) / 256, 256>>>(*cam, n, d, d + 9 * m, d + 2 * m, d + 5 * m, d + 7 * m);
    HIPCHK(hipDeviceSynchronize());
    if (ray_out) HIPCHK(d.download(ray_out, (size_t)3 * n, 2 * m));
    if (un_out) HIPCHK(d.download(un_out, (size_t)2 * n, 5 * m));
    if (uv_out) HIPCHK(d.download(uv_out, (size_t)2 * n, 7 * m));
    return VIO_OK;
}

static int stage_relative_r_impl(int n, const double *corres6, double *R9, int *detail8) {
    if (n < 0 || (n > 0 && !corres6) || !R9) return VIO_EINVAL;
    DevBuf<double> dc, dR;
    DevBuf<int> dd;
    const size_t lds = (size_t)n * 40 + 64;   // four coordinate arrays + the RANSAC status flags
    // refused before anything is asked of the runtime: a limit it cannot grant would stay behind as the thread's last error
    if (!lds_fits((const void *)be_stage_relative_r_kernel, lds, "be_stage_relative_r")) return VIO_ECAPACITY;
    HIPCHK(dc.alloc((size_t)6 * (n + 1)));
    HIPCHK(dR.alloc(9));
    if (n > 0) HIPCHK(dc.upload(corres6, (size_t)6 * n));
    (void)raise_lds_limit((const void *)be_stage_relative_r_kernel, lds);
    if (detail8) HIPCHK(dd.alloc(8));
    be_stage_relative_r_kernel<<<1, 256, lds>>>(n, dc, dR, detail8 ? (int *)dd : nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dR.download(R9, 9));
    if (detail8) HIPCHK(dd.download(detail8, 8));
    return VIO_OK;
}
int vio_stage_relative_r(int n, const double *corres6, double *R9) { return stage_relative_r_impl(n, corres6, R9, nullptr); }
int vio_stage_relative_r_detail(int n, const double *corres6, double *R9, int *detail8) {
    if (!detail8) return VIO_EINVAL;
    return stage_relative_r_impl(n, corres6, R9, detail8);
}

static int stage_imu_impl(const vio_config *cfg, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                          const double *gyr0, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                          const double *pose_j, const double *sb_j, double *preint_out, double *r15, double *J480, double *G961) {
    DevBuf<double> dG, dbuf;
    DevBuf<PreInt> dp;
    std::vector<PreInt> hpv(1);
    PreInt *hp = hpv.data();
    std::vector<double> hb;
    memset(hp, 0, sizeof(PreInt));
    {
        using namespace dm;
        // IntegrationBase constructor on the host side of the test harness (plain state initialisation)
        for (int k = 0; k < 3; k++) { hp->lin_acc[k] = acc0[k]; hp->lin_gyr[k] = gyr0[k]; hp->lin_ba[k] = ba[k]; hp->lin_bg[k] = bg[k]; hp->acc0[k] = acc0[k]; hp->gyr0[k] = gyr0[k]; }
        hp->dq[0] = 1;
        for (int i = 0; i < 15; i++) hp->jac[i * 16] = 1;
        hp->valid = 1;
    }
    size_t nd = (size_t)n * 7 + 32 + 461 + 15 + 480;
    hb.assign(nd, 0.0);
    for (int i = 0; i < n; i++) { hb[i] = dt[i]; for (int k = 0; k < 3; k++) { hb[n + 3 * i + k] = acc[3 * i + k]; hb[4 * n + 3 * i + k] = gyr[3 * i + k]; } }
    for (int k = 0; k < 7; k++) { hb[7 * n + k] = pose_i[k]; hb[7 * n + 16 + k] = pose_j[k]; }
    for (int k = 0; k < 9; k++) { hb[7 * n + 7 + k] = sb_i[k]; hb[7 * n + 23 + k] = sb_j[k]; }
    HIPCHK(dp.alloc(1));
    HIPCHK(dbuf.alloc(nd));
    HIPCHK(dp.upload(hp, 1));
    HIPCHK(dbuf.upload(hb.data(), nd));
    be_stage_imu_kernel<<<1, 256>>>(*cfg, dp, n, dbuf, dbuf + n, dbuf + 4 * n, dbuf + 7 * n, cfg->g_norm, dbuf + 7 * n + 32, dbuf + 7 * n + 32 + 461,
                                    dbuf + 7 * n + 32 + 461 + 15);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dbuf.download(hb.data(), nd));
    if (preint_out) memcpy(preint_out, &hb[7 * n + 32], 461 * sizeof(double));
    if (r15) memcpy(r15, &hb[7 * n + 32 + 461], 15 * sizeof(double));
    if (J480) memcpy(J480, &hb[7 * n + 32 + 461 + 15], 480 * sizeof(double));
    if (G961) {
        HIPCHK(dG.alloc(961));
        HIPCHK(hipMemset(dG, 0, 961 * sizeof(double)));
        be_stage_imu_block_kernel<<<1, 64>>>(dp, dbuf + 7 * n, cfg->g_norm, dG);
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(dG.download(G961, 961));
    }
    return VIO_OK;
}

int vio_stage_imu_factor(const vio_config *cfg, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                         const double *gyr0, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                         const double *pose_j, const double *sb_j, double *preint_out, double *r15, double *J480) {
    return stage_imu_impl(cfg, n, dt, acc, gyr, acc0, gyr0, ba, bg, pose_i, sb_i, pose_j, sb_j, preint_out, r15, J480, nullptr);
}
int vio_stage_imu_block(const vio_config *cfg, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                        const double *gyr0, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                        const double *pose_j, const double *sb_j, double *G961) {
    return stage_imu_impl(cfg, n, dt, acc, gyr, acc0, gyr0, ba, bg, pose_i, sb_i, pose_j, sb_j, nullptr, nullptr, nullptr, G961);
}

// IntegrationBase constructor on the host side of the test harnesses (plain state initialisation)
static void stage_preint_init(PreInt *hp, const double *acc0, const double *gyr0, const double *ba, const double *bg) {
    memset(hp, 0, sizeof(PreInt));
    for (int k = 0; k < 3; k++) { hp->lin_acc[k] = acc0[k]; hp->lin_gyr[k] = gyr0[k]; hp->lin_ba[k] = ba[k]; hp->lin_bg[k] = bg[k]; hp->acc0[k] = acc0[k]; hp->gyr0[k] = gyr0[k]; }
    hp->dq[0] = 1;
    for (int i = 0; i < 15; i++) hp->jac[i * 16] = 1;
    hp->valid = 1;
}

// world31 != NULL (vio_stage_preint_ring): dt / acc / gyr are a ring of na entries, n samples from `head` on; world31 in and out
static int stage_preint_impl(const vio_config *cfg, int mode, int n, int na, const double *dt, const double *acc, const double *gyr, int head,
                             double prev_time, double cur_time, double *world31, const double *acc0, const double *gyr0, const double *ba,
                             const double *bg, double *out686, int *n_buf_out, double *buf_out) {
    if (!cfg || n < 0 || (na > 0 && (!dt || !acc || !gyr)) || !acc0 || !gyr0 || !ba || !bg || !out686) return VIO_EINVAL;
    DevBuf<double> dbuf;
    DevBuf<PreInt> dp;
    std::vector<PreInt> hpv(1);
    PreInt *hp = hpv.data();
    stage_preint_init(hp, acc0, gyr0, ba, bg);
    const size_t nd = (size_t)na * 7 + 686 + 31;
    std::vector<double> hb(nd, 0.0);
    for (int i = 0; i < na; i++) { hb[i] = dt[i]; for (int k = 0; k < 3; k++) { hb[na + 3 * i + k] = acc[3 * i + k]; hb[4 * na + 3 * i + k] = gyr[3 * i + k]; } }
    if (world31) memcpy(&hb[7 * (size_t)na + 686], world31, 31 * sizeof(double));
    HIPCHK(dp.alloc(1));
    HIPCHK(dbuf.alloc(nd));
    HIPCHK(dp.upload(hp, 1));
    HIPCHK(dbuf.upload(hb.data(), nd));
    if (world31) be_stage_preint_ring_kernel<<<1, 256>>>(*cfg, dp, PreintRing{dbuf, dbuf + na, dbuf + 4 * na, head, na, prev_time, cur_time, n}, dbuf + 7 * na + 686, dbuf + 7 * na);
    else be_stage_preint_kernel<<<1, 256>>>(*cfg, dp, n, dbuf, dbuf + na, dbuf + 4 * na, mode, dbuf + 7 * na);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dbuf.download(hb.data(), nd));
    HIPCHK(dp.download(hp, 1));
    memcpy(out686, &hb[7 * (size_t)na], 686 * sizeof(double));
    if (world31) memcpy(world31, &hb[7 * (size_t)na + 686], 31 * sizeof(double));
    if (n_buf_out) *n_buf_out = hp->n_buf;
    if (buf_out)
        for (int q = 0; q < VIO_IMU_SLOT_CAP; q++) {
            buf_out[7 * q] = hp->dt_buf[q];
            for (int k = 0; k < 3; k++) { buf_out[7 * q + 1 + k] = hp->acc_buf[q][k]; buf_out[7 * q + 4 + k] = hp->gyr_buf[q][k]; }
        }
    return VIO_OK;
}
int vio_stage_preint(const vio_config *cfg, int mode, int n, const double *dt, const double *acc, const double *gyr, const double *acc0,
                     const double *gyr0, const double *ba, const double *bg, double *out686, int *n_buf_out, double *buf_out) {
    if (mode < 0 || mode > 2) return VIO_EINVAL;
    return stage_preint_impl(cfg, mode, n, n, dt, acc, gyr, 0, 0, 0, nullptr, acc0, gyr0, ba, bg, out686, n_buf_out, buf_out);
}
int vio_stage_preint_ring(const vio_config *cfg, int n, int head, int cap, const double *t, const double *acc, const double *gyr, double prev_time,
                          double cur_time, double *world31, const double *acc0, const double *gyr0, const double *ba, const double *bg,
                          double *out686, int *n_buf_out, double *buf_out) {
    if (n < 1 || head < 0 || cap < 1 || !world31) return VIO_EINVAL;
    return stage_preint_impl(cfg, 2, n, cap, t, acc, gyr, head, prev_time, cur_time, world31, acc0, gyr0, ba, bg, out686, n_buf_out, buf_out);
}

int vio_stage_imu_raw(const vio_config *cfg, const double *pre461, const double *ba, const double *bg, const double *pose_i, const double *sb_i,
                      const double *pose_j, const double *sb_j, double *r15, double *J450, double *Jp465) {
    if (!cfg || !pre461 || !ba || !bg || !pose_i || !sb_i || !pose_j || !sb_j || !r15 || !J450 || !Jp465) return VIO_EINVAL;
    DevBuf<double> db;
    DevBuf<PreInt> dp;
    std::vector<PreInt> hpv(1);
    PreInt *hp = hpv.data();
    const double z3[3] = {0, 0, 0};
    stage_preint_init(hp, z3, z3, ba, bg);
    for (int k = 0; k < 3; k++) { hp->dp[k] = pre461[k]; hp->dv[k] = pre461[7 + k]; }
    for (int k = 0; k < 4; k++) hp->dq[k] = pre461[3 + k];
    hp->sum_dt = pre461[10];
    for (int k = 0; k < 225; k++) { hp->jac[k] = pre461[11 + k]; hp->cov[k] = pre461[236 + k]; }
    double hb[32 + 15 + 450 + 465];
    memset(hb, 0, sizeof(hb));
    memcpy(hb, pose_i, 56); memcpy(hb + 7, sb_i, 72); memcpy(hb + 16, pose_j, 56); memcpy(hb + 23, sb_j, 72);
    memcpy(hb + 32 + 15 + 450, Jp465, 465 * sizeof(double));
    HIPCHK(dp.alloc(1));
    HIPCHK(db.alloc(32 + 15 + 450 + 465));
    HIPCHK(dp.upload(hp, 1));
    HIPCHK(db.upload(hb, 32 + 15 + 450 + 465));
    be_stage_imu_raw_kernel<<<1, 64>>>(dp, db, cfg->g_norm, db + 32, db + 47, db + 497);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(db.download(hb, 32 + 15 + 450 + 465));
    memcpy(r15, hb + 32, 15 * sizeof(double));
    memcpy(J450, hb + 47, 450 * sizeof(double));
    memcpy(Jp465, hb + 497, 465 * sizeof(double));
    return VIO_OK;
}

int vio_stage_projection_pair(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep, double td,
                              const double *obs_i, const double *obs_j, int use_td, int cauchy, int rs, int ext, double *r2, double *wgt,
                              double *J, int nJ) {
    if (!cfg || !pose_i || !pose_j || !ex || !obs_i || !obs_j || !r2 || !wgt || !J) return VIO_EINVAL;
    if (!((rs == 20) || (rs == 14 && !ext)) || nJ < 2 * rs || nJ > 4096) return VIO_EINVAL;   // ext writes columns 12 .. 19 of both rows
    std::vector<double> hb((size_t)41 + 3 + nJ);
    DevBuf<double> db;
    memcpy(&hb[0], pose_i, 56); memcpy(&hb[7], pose_j, 56); memcpy(&hb[14], ex, 56);
    hb[21] = inv_dep; hb[22] = td;
    memcpy(&hb[23], obs_i, 72); memcpy(&hb[32], obs_j, 72);
    hb[41] = r2[0]; hb[42] = r2[1]; hb[43] = *wgt;
    memcpy(&hb[44], J, (size_t)nJ * sizeof(double));
    HIPCHK(db.alloc(hb.size()));
    HIPCHK(db.upload(hb.data(), hb.size()));
    be_stage_projection_pair_kernel<<<1, 64>>>(*cfg, db, use_td, cauchy, rs, ext, db + 41, db + 43, db + 44);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(db.download(hb.data(), hb.size()));
    r2[0] = hb[41]; r2[1] = hb[42]; *wgt = hb[43];
    memcpy(J, &hb[44], (size_t)nJ * sizeof(double));
    return VIO_OK;
}

int vio_stage_pose_ops(int n, const double *x7, const double *d6, const double *x07, double *plus7, double *dx6) {
    if (n < 0 || (n > 0 && (!x7 || !d6 || !x07 || !plus7 || !dx6))) return VIO_EINVAL;
    if (n == 0) return VIO_OK;
    DevBuf<double> db;
    const size_t m = (size_t)n;   // x7 d6 x07 plus7 dx6
    std::vector<double> hb(33 * m, 0.0);
    memcpy(&hb[0], x7, 7 * m * sizeof(double)); memcpy(&hb[7 * m], d6, 6 * m * sizeof(double)); memcpy(&hb[13 * m], x07, 7 * m * sizeof(double));
    HIPCHK(db.alloc(33 * m));
    HIPCHK(db.upload(hb.data(), 33 * m));
    be_stage_pose_ops_kernel<<<(n + 63) / 64, 64>>>(n, db, db + 7 * m, db + 13 * m, db + 20 * m, db + 27 * m);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(db.download(hb.data(), 33 * m));
    memcpy(plus7, &hb[20 * m], 7 * m * sizeof(double));
    memcpy(dx6, &hb[27 * m], 6 * m * sizeof(double));
    return VIO_OK;
}

static int stage_projection_impl(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep, double td,
                                 const double *obs_i, const double *obs_j, int use_td, int form, double *r2, double *J46) {
    double hb[41 + 2 + 46];
    DevBuf<double> db;
    memcpy(hb, pose_i, 56); memcpy(hb + 7, pose_j, 56); memcpy(hb + 14, ex, 56);
    hb[21] = inv_dep; hb[22] = td;
    memcpy(hb + 23, obs_i, 72); memcpy(hb + 32, obs_j, 72);
    HIPCHK(db.alloc(41 + 2 + 46));
    HIPCHK(db.upload(hb, 41 + 2 + 46));
    be_stage_projection_kernel<<<1, 64>>>(*cfg, db, use_td, form, db + 41, db + 43);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(db.download(hb, 41 + 2 + 46));
    memcpy(r2, hb + 41, 16);
    memcpy(J46, hb + 43, 46 * 8);
    return VIO_OK;
}
// cv::solvePnP(SOLVEPNP_ITERATIVE, useExtrinsicGuess = 1) with K = I as FeatureManager::solvePoseByPnP calls it (feature_manager.cpp:571):
// obj[n][3], img[n][2] (both rounded to float like cv::Point3f / Point2f), rvec / tvec in and out
static int stage_pnp_impl(int n, const double *obj, const double *img, double *rvec3, double *tvec3, int *trace4) {
    if (n < 4 || !obj || !img || !rvec3 || !tvec3) return VIO_EINVAL;
    std::vector<double> pts((size_t)n * 5), par(6);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) pts[5 * i + k] = (double)(float)obj[3 * i + k];
        for (int k = 0; k < 2; k++) pts[5 * i + 3 + k] = (double)(float)img[2 * i + k];
    }
    for (int k = 0; k < 3; k++) { par[k] = rvec3[k]; par[3 + k] = tvec3[k]; }
    DevBuf<double> dp, dq;
    HIPCHK(dp.alloc(pts.size()));
    HIPCHK(dq.alloc(6));
    HIPCHK(dp.upload(pts.data(), pts.size()));
    HIPCHK(dq.upload(par.data(), 6));
    DevBuf<int> dt;
    if (trace4) HIPCHK(dt.alloc(4));
    be_stage_pnp_kernel<<<1, 256>>>(dp, n, dq, trace4 ? (int *)dt : nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dq.download(par.data(), 6));
    if (trace4) HIPCHK(dt.download(trace4, 4));
    for (int k = 0; k < 3; k++) { rvec3[k] = par[k]; tvec3[k] = par[3 + k]; }
    return VIO_OK;
}
int vio_stage_pnp(int n, const double *obj, const double *img, double *rvec3, double *tvec3) { return stage_pnp_impl(n, obj, img, rvec3, tvec3, nullptr); }
int vio_stage_pnp_trace(int n, const double *obj, const double *img, double *rvec3, double *tvec3, int *trace4) {
    if (!trace4) return VIO_EINVAL;
    return stage_pnp_impl(n, obj, img, rvec3, tvec3, trace4);
}
// cv::Rodrigues of the device solvePnP, one thread per item: mode 0 in = r[n][3], out[n][36] = R, dR/dr; mode 1 in = R[n][9], out = r[n][3]
int vio_stage_rodrigues(int mode, int n, const double *in, double *out) {
    if (mode < 0 || mode > 1 || n < 0 || (n > 0 && (!in || !out))) return VIO_EINVAL;
    if (n == 0) return VIO_OK;
    const size_t ni = (size_t)n * (mode == 0 ? 3 : 9), no = (size_t)n * (mode == 0 ? 36 : 3);
    DevBuf<double> di, dout;
    HIPCHK(di.alloc(ni));
    HIPCHK(dout.alloc(no));
    HIPCHK(di.upload(in, ni));
    be_stage_rodrigues_kernel<<<(n + 63) / 64, 64>>>(mode, n, di, dout);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dout.download(out, no));
    return VIO_OK;
}

// The literal marginalisation, one part at a time (kernels.h MargLiteralStage).  One scratch allocation holds every array the device code reads or
// writes, each followed (the first also preceded) by MARG_STAGE_GUARD guard words; the whole allocation starts out as guard words, so an output the
// kernel did not write shows as such.
#define MARG_STAGE_GUARD 32
int vio_stage_marg_literal(int part, int md, int F0, int n, int ldc, int nt, int mxl, int pinv_direct, int second_new, const double *A, const double *b,
                           const double *Cl, const double *Hll, const double *gl, double *Ainv_out, double *Ar_out, double *br_out, double *J_out,
                           double *rf_out, double *H_out, double *r_out, double *scal2_out, int *info8_out) {
    if (part < 0 || part > 2 || (md != 6 && md != 15) || F0 < 0 || F0 > 480 || n < 1 || n > 6 * VIO_MAXW + 16 || (nt != 256 && nt != 512) || mxl < 0 ||
        mxl > 128 || !A || !scal2_out || !info8_out)
        return VIO_EINVAL;
    const size_t m = (size_t)md + F0, mq = (size_t)md + n, N = (size_t)n;
    if (part == 0 && (!b || ldc < (int)mq || (F0 > 0 && (!Cl || !Hll || !gl)) || !Ainv_out || !Ar_out || !br_out)) return VIO_EINVAL;
    if (part == 1 && !b) return VIO_EINVAL;
    if (part <= 1 && (!J_out || !rf_out || !H_out || !r_out)) return VIO_EINVAL;
    if (part == 2 && (ldc < md || (F0 > 0 && (!Cl || !Hll)))) return VIO_EINVAL;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const int mxl_eff = mxl > 0 ? mxl : marg_exact_mxl(dev);
    const size_t lds = std::max(marg_exact_lds_bytes(mxl_eff), marg_exact_hbm_lds_bytes());
    if (!lds_fits((const void *)be_stage_marg_literal_kernel, lds, "be_stage_marg_literal")) return VIO_EINVAL;
    // segment sizes in doubles (0 where the part does not touch the array)
    enum { S_A, S_B, S_CL, S_HLL, S_GL, S_MARGE, S_MARGV, S_MARGW, S_VEC, S_PJ, S_PH, S_PR, S_PRF, S_SCAL, S_COUNT };
    size_t sz[S_COUNT] = {0}, off[S_COUNT];
    const bool lm = part != 1 && F0 > 0;
    sz[S_A] = part == 0 ? mq * mq : part == 2 ? (size_t)md * md : 0;
    sz[S_B] = part == 0 ? mq : 0;
    sz[S_CL] = lm ? (size_t)F0 * ldc : 0; sz[S_HLL] = lm ? (size_t)F0 : 0; sz[S_GL] = lm && part == 0 ? (size_t)F0 : 0;
    sz[S_MARGE] = part == 0 ? 3 * m * m + N * m : 0;   // as the handle sizes it, MX = m
    if (part <= 1) { sz[S_MARGV] = N * N; sz[S_MARGW] = (N + 16) * (N + 16); sz[S_VEC] = N; sz[S_PJ] = N * N; sz[S_PH] = N * N; sz[S_PR] = N; sz[S_PRF] = N; }
    sz[S_SCAL] = 2;
    size_t total = MARG_STAGE_GUARD;
    for (int k = 0; k < S_COUNT; k++) { off[k] = total; total += sz[k] + MARG_STAGE_GUARD; }
    const double gval = -1.2345678901234567e300;
    std::vector<double> hb(total, gval);
    auto put = [&](int seg, const double *src, size_t count) { if (count) memcpy(&hb[off[seg]], src, count * sizeof(double)); };
    if (part == 0) { put(S_A, A, mq * mq); put(S_B, b, mq); put(S_GL, gl, sz[S_GL]); }
    if (part == 1) { put(S_MARGV, A, N * N); put(S_VEC, b, N); }
    if (part == 2) put(S_A, A, (size_t)md * md);
    put(S_CL, Cl, sz[S_CL]); put(S_HLL, Hll, sz[S_HLL]);
    DevCfg hc;
    memset(&hc, 0, sizeof(hc));
    hc.MX = part == 0 ? (int)m : 0; hc.MXL = mxl_eff;
    std::vector<BeSeq> hbe(1);
    memset(hbe.data(), 0, sizeof(BeSeq));
    for (int k = 0; k < 16; k++) hbe[0].dbg[k] = -1;
    int hinfo[4] = {0, -1, -1, -1};
    DevBuf<double> dbuf;
    DevBuf<DevCfg> dcfg;
    DevBuf<BeSeq> dbe;
    DevBuf<int> dinfo;
    HIPCHK(dbuf.alloc(total)); HIPCHK(dcfg.alloc(1)); HIPCHK(dbe.alloc(1)); HIPCHK(dinfo.alloc(4));
    HIPCHK(dbuf.upload(hb.data(), total)); HIPCHK(dcfg.upload(&hc, 1)); HIPCHK(dbe.upload(hbe.data(), 1)); HIPCHK(dinfo.upload(hinfo, 4));
    MargLiteralStage a;
    memset(&a, 0, sizeof(a));
    double *d = dbuf;
    a.cfg = dcfg; a.be = dbe; a.info = dinfo;
    a.A = d + off[S_A]; a.b = d + off[S_B]; a.Cl = d + off[S_CL]; a.Hll = d + off[S_HLL]; a.gl = d + off[S_GL];
    a.margE = d + off[S_MARGE]; a.margV = d + off[S_MARGV]; a.margW = d + off[S_MARGW]; a.vec = d + off[S_VEC];
    a.prior_J = d + off[S_PJ]; a.prior_H = d + off[S_PH]; a.prior_r = d + off[S_PR]; a.prior_rf = d + off[S_PRF]; a.scal = d + off[S_SCAL];
    a.part = part; a.md = md; a.F0 = F0; a.n = n; a.ldc = ldc; a.pinv_direct = pinv_direct; a.second_new = second_new;
    (void)raise_lds_limit((const void *)be_stage_marg_literal_kernel, lds);
    be_stage_marg_literal_kernel<<<1, nt, lds>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> in(hb);
    HIPCHK(dbuf.download(hb.data(), total)); HIPCHK(dinfo.download(hinfo, 4));
    int good = 1;
    for (size_t q = 0; q < MARG_STAGE_GUARD; q++) if (memcmp(&hb[q], &gval, sizeof(double)) != 0) good = 0;
    for (int k = 0; k < S_COUNT; k++)
        for (size_t q = 0; q < MARG_STAGE_GUARD; q++) if (memcmp(&hb[off[k] + sz[k] + q], &gval, sizeof(double)) != 0) good = 0;
    // the inputs the device code only reads
    for (int k : {(int)S_A, (int)S_B, (int)S_CL, (int)S_HLL, (int)S_GL})
        if (sz[k] && memcmp(&hb[off[k]], &in[off[k]], sz[k] * sizeof(double)) != 0) good = 0;
    auto get = [&](double *dst, size_t from, size_t count) { if (dst && count) memcpy(dst, &hb[from], count * sizeof(double)); };
    if (part == 0) { get(Ainv_out, off[S_MARGE] + 2 * m * m, m * m); get(Ar_out, off[S_MARGV], N * N); get(br_out, off[S_VEC], N); }
    if (part <= 1) { get(J_out, off[S_PJ], N * N); get(rf_out, off[S_PRF], N); get(H_out, off[S_PH], N * N); get(r_out, off[S_PR], N); }
    scal2_out[0] = hb[off[S_SCAL]]; scal2_out[1] = hb[off[S_SCAL] + 1];
    info8_out[0] = mxl_eff; info8_out[1] = good; info8_out[2] = hinfo[0]; info8_out[3] = hinfo[1]; info8_out[4] = hinfo[2]; info8_out[5] = hinfo[3];
    info8_out[6] = 0; info8_out[7] = 0;
    return VIO_OK;
}

// ---- the default marginalisation on a staged state, through the handle's own kernels (include/vio_abi.h vio_debug_marg_set / _run / _get)
static bool all_finite(const double *p, size_t n) {
    for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false;
    return true;
}
#define MARG_STAGE_REFUSE(msg) do { g_err = std::string(who) + ": " + (msg); return VIO_EINVAL; } while (0)
// The validation vio_debug_marg_set and vio_debug_solve_set share: everything a kernel of either stage indexes with.  Writes nothing; live[slot] = the
// slot is in the list.  solve: also what only the solver indexes with (include/vio_abi.h vio_debug_solve_set).
static int stage_validate(const vio_batch *h, const vio_marg_stage_in *in, const char *who, bool solve, std::vector<char> &live) {
    const DevCfg &C = h->hc;
    const int W = C.W, W1 = W + 1, NL = C.NL, n = C.NPRIOR;
    const vio_publish_tables &t = in->t;
    if (!t.lm_order || !t.lm_id || !t.lm_start || !t.lm_nobs || !t.lm_solve_flag || !t.lm_dyn || !t.lm_depth || !t.lm_obs || !t.Ps || !t.Rs || !t.Headers ||
        !t.ric || !t.tic || !in->lm_est_flag || !in->Vs || !in->Bas || !in->Bgs || !in->g || !in->pre_idx)
        MARG_STAGE_REFUSE("a table is missing");
    if (in->n_lm < 0 || in->n_lm > NL) MARG_STAGE_REFUSE("n_lm outside 0 .. NL");
    if (in->ring_base < 0 || in->ring_base > W) MARG_STAGE_REFUSE("ring_base outside 0 .. W");
    if ((in->marginalization_flag | in->has_prior) & ~1) MARG_STAGE_REFUSE("marginalization_flag and has_prior are 0 or 1");
    live.assign(NL, 0);
    int F0 = 0;
    long long nres = 0;
    for (int k = 0; k < in->n_lm; k++) {
        const int slot = t.lm_order[k];
        if (slot < 0 || slot >= NL) MARG_STAGE_REFUSE("lm_order names a slot >= NL");
        if (live[slot]) MARG_STAGE_REFUSE("lm_order names a slot twice");
        live[slot] = 1;
        const int st = t.lm_start[slot], no = t.lm_nobs[slot];
        if (st < 0 || st > W) MARG_STAGE_REFUSE("lm_start outside 0 .. W");
        if (no < 1 || no > W1 - st) MARG_STAGE_REFUSE("lm_nobs outside 1 .. W + 1 - lm_start");
        if (!std::isfinite(t.lm_depth[slot])) MARG_STAGE_REFUSE("a depth is not finite");
        if (!all_finite(t.lm_obs + (size_t)slot * W1 * VIO_OBS_D, (size_t)W1 * VIO_OBS_D)) MARG_STAGE_REFUSE("an observation is not finite");
        if (!t.lm_dyn[slot] && no >= 2 && st < W - 2 && st == 0) F0++;
        if (!t.lm_dyn[slot] && no >= 2 && st < W - 2) nres += no - 1;
        if (solve && (in->lm_est_flag[slot] < 0 || in->lm_est_flag[slot] > 2)) MARG_STAGE_REFUSE("lm_est_flag outside 0 .. 2");
    }
    if (solve) {
        // (landmarks in the problem <= n_lm <= NL by the checks above; the next test cannot fire at today's sizing either, NRES >= W NP + 2 NL: it is
        // there for the day the sizing changes)
        if (nres > (long long)C.NRES - 2 * NL) MARG_STAGE_REFUSE("more projection residuals than the NRES - 2 NL records of the residual list");
        // (ps_setup asks for 3 + ceil(nres / (256 eval_rpt)) evaluation workgroups; the launch has ps_eval_blocks: a solve beyond them would never be accepted)
        if (h->solve_mode == 1 && nres > (long long)(h->ps_eval_blocks - 3) * 256 * h->B.eval_rpt)
            MARG_STAGE_REFUSE("more projection residuals than the handle's evaluation launch covers");
    }
    if (F0 > C.NRES / W) MARG_STAGE_REFUSE("more landmarks start in frame 0 than NRES / W residual records hold");
    for (int i = 1; i <= W; i++) if (!(t.Headers[i] > t.Headers[i - 1])) MARG_STAGE_REFUSE("Headers must increase");
    if (!all_finite(t.Headers, W1) || !all_finite(t.Ps, 3 * (size_t)W1) || !all_finite(t.Rs, 9 * (size_t)W1) || !all_finite(in->Vs, 3 * (size_t)W1) ||
        !all_finite(in->Bas, 3 * (size_t)W1) || !all_finite(in->Bgs, 3 * (size_t)W1) || !all_finite(t.ric, 9) || !all_finite(t.tic, 3) ||
        !all_finite(in->g, 3) || !std::isfinite(in->td))
        MARG_STAGE_REFUSE("a window state is not finite");
    {
        std::vector<char> seen(W1, 0);
        for (int i = 0; i <= W; i++) {
            const int p = in->pre_idx[i];
            if (p < 0 || p > W || seen[p]) MARG_STAGE_REFUSE("pre_idx must be a permutation of 0 .. W");
            seen[p] = 1;
        }
    }
    if (in->has_prior) {
        if (!in->prior_present || !in->prior_H || !in->prior_r || !in->prior_x0) MARG_STAGE_REFUSE("has_prior without a prior");
        for (int i = 0; i < W + 3; i++) if (in->prior_present[i] & ~1) MARG_STAGE_REFUSE("prior_present holds 0 or 1");
        if (!all_finite(in->prior_H, (size_t)n * n) || !all_finite(in->prior_r, n) || !all_finite(in->prior_x0, (size_t)W * 7 + 17))
            MARG_STAGE_REFUSE("the prior is not finite");
    }
    if (C.c.use_imu) {
        if (!in->imu_n || !in->imu_dt || !in->imu_acc || !in->imu_gyr || !in->imu_acc0 || !in->imu_gyr0 || !in->imu_ba || !in->imu_bg)
            MARG_STAGE_REFUSE("an IMU table is missing");
        for (int j = 1; j <= W; j++) {
            const int ns = in->imu_n[j];
            if (ns < 0 || ns > VIO_IMU_SLOT_CAP) MARG_STAGE_REFUSE("more than 64 samples in an interval");
            const size_t o = (size_t)j * VIO_IMU_SLOT_CAP;
            if (!all_finite(in->imu_dt + o, ns) || !all_finite(in->imu_acc + 3 * o, 3 * (size_t)ns) || !all_finite(in->imu_gyr + 3 * o, 3 * (size_t)ns) ||
                !all_finite(in->imu_acc0 + 3 * j, 3) || !all_finite(in->imu_gyr0 + 3 * j, 3) || !all_finite(in->imu_ba + 3 * j, 3) ||
                !all_finite(in->imu_bg + 3 * j, 3))
                MARG_STAGE_REFUSE("an IMU sample is not finite");
        }
    }
    return VIO_OK;
}
#undef MARG_STAGE_REFUSE

// A validated state (stage_validate) into the handle's arrays.  solve: the state in front of a solve (vio_debug_solve_set) instead of the one in front
// of a marginalisation.
static int stage_write(vio_batch *h, int seq, const vio_marg_stage_in *in, const std::vector<char> &live, bool solve) {
    const DevCfg &C = h->hc;
    Batch &B = h->B;
    const int W = C.W, W1 = W + 1, NL = C.NL, n = C.NPRIOR;
    const vio_publish_tables &t = in->t;
    const bool imu = C.c.use_imu != 0;
    // ---- the window state
    std::vector<BeSeq> bev(1);
    BeSeq &be = bev[0];
    HIPCHK(hipMemcpy(&be, B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    for (int i = 0; i <= W; i++) {
        for (int k = 0; k < 3; k++) { be.Ps[i][k] = t.Ps[3 * i + k]; be.Vs[i][k] = in->Vs[3 * i + k]; be.Bas[i][k] = in->Bas[3 * i + k]; be.Bgs[i][k] = in->Bgs[3 * i + k]; }
        for (int k = 0; k < 9; k++) be.Rs[i][k] = t.Rs[9 * i + k];
        be.Headers[i] = t.Headers[i];
        be.pre_idx[i] = in->pre_idx[i];
    }
    for (int k = 0; k < 9; k++) be.ric[k] = t.ric[k];
    for (int k = 0; k < 3; k++) { be.tic[k] = t.tic[k]; be.g[k] = in->g[k]; }
    be.td = in->td;
    be.frame_count = W; be.do_marg = solve ? 0 : 1; be.rebooted = 0; be.processed = 0;
    if (solve) {
        be.do_solve = 1; be.solver_flag = 1; be.openExEstimation = 0; be.relo_info = 0; be.init_frame = 0; be.overflow = 0;
        // what failureDetection at the end of the solve compares the new window with: as the previous frame left them
        for (int k = 0; k < 3; k++) { be.last_P[k] = t.Ps[3 * W + k]; be.last_P0[k] = t.Ps[k]; }
        for (int k = 0; k < 9; k++) { be.last_R[k] = t.Rs[9 * W + k]; be.last_R0[k] = t.Rs[k]; }
    }
    be.marginalization_flag = in->marginalization_flag;
    be.has_prior = in->has_prior;
    for (int i = 0; i < VIO_MAXW + 3; i++) be.prior_present[i] = (in->has_prior && i < W + 3) ? in->prior_present[i] : 0;
    be.ring_base = in->ring_base;
    be.n_lm = in->n_lm;
    be.n_free = NL - in->n_lm;
    for (int k = 0; k < 16; k++) be.dbg[k] = -1;
    // ---- the landmark tables (the free list as init_state orders it: the lowest free slot is handed out first)
    const size_t o = (size_t)seq * NL;
    std::vector<int> fr;
    for (int slot = NL - 1; slot >= 0; slot--) if (!live[slot]) fr.push_back(slot);
    fr.resize(NL, 0);
    std::vector<int> ord(NL, 0);
    for (int k = 0; k < in->n_lm; k++) ord[k] = t.lm_order[k];
    HIPCHK(hipMemcpy(B.lm_order + o, ord.data(), NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_free + o, fr.data(), NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_id + o, t.lm_id, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_start + o, t.lm_start, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_nobs + o, t.lm_nobs, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_dyn + o, t.lm_dyn, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_solve_flag + o, t.lm_solve_flag, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_est_flag + o, in->lm_est_flag, NL * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_depth + o, t.lm_depth, NL * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.lm_obs + o * W1 * VIO_OBS_D, t.lm_obs, (size_t)NL * W1 * VIO_OBS_D * sizeof(double), hipMemcpyHostToDevice));
    // ---- the prior
    if (in->has_prior) {
        HIPCHK(hipMemcpy(B.prior_H + (size_t)seq * n * n, in->prior_H, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(B.prior_r + (size_t)seq * n, in->prior_r, n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(B.prior_x0 + (size_t)seq * (W * 7 + 17), in->prior_x0, ((size_t)W * 7 + 17) * sizeof(double), hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemset(B.prior_H + (size_t)seq * n * n, 0, (size_t)n * n * sizeof(double)));
        HIPCHK(hipMemset(B.prior_r + (size_t)seq * n, 0, n * sizeof(double)));
        HIPCHK(hipMemset(B.prior_x0 + (size_t)seq * (W * 7 + 17), 0, ((size_t)W * 7 + 17) * sizeof(double)));
    }
    be.prior_c0 = 0;
    HIPCHK(hipMemcpy(B.be + seq, &be, sizeof(BeSeq), hipMemcpyHostToDevice));
    // ---- the pre-integrations, by the pipeline's routine on the raw samples
    if (imu) {
        vio_config cs = C.c;   // the handle's configuration with the sequence's noise densities
        cal_into_config(h->cal[seq], cs);
        DevBuf<double> dbuf;
        const size_t cap = VIO_IMU_SLOT_CAP;
        HIPCHK(dbuf.alloc(7 * cap + 686));
        std::vector<PreInt> hpv(1);
        for (int j = 1; j <= W; j++) {
            const int ns = in->imu_n[j];
            PreInt *dp = B.pre + (size_t)seq * (W + 2) + in->pre_idx[j];
            stage_preint_init(hpv.data(), in->imu_acc0 + 3 * j, in->imu_gyr0 + 3 * j, in->imu_ba + 3 * j, in->imu_bg + 3 * j);
            HIPCHK(hipMemcpy(dp, hpv.data(), sizeof(PreInt), hipMemcpyHostToDevice));
            if (ns > 0) {
                HIPCHK(dbuf.upload(in->imu_dt + (size_t)j * cap, ns));
                HIPCHK(dbuf.upload(in->imu_acc + 3 * (size_t)j * cap, 3 * (size_t)ns, cap));
                HIPCHK(dbuf.upload(in->imu_gyr + 3 * (size_t)j * cap, 3 * (size_t)ns, 4 * cap));
            }
            be_stage_preint_kernel<<<1, 256>>>(cs, dp, ns, dbuf, dbuf + cap, dbuf + 4 * cap, 2, dbuf + 7 * cap);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipDeviceSynchronize());
    }
    return VIO_OK;
}

int vio_debug_marg_set(vio_batch *h, int seq, const vio_marg_stage_in *in) {
    VIO_ENTER(h, seq, true);
    if (!in) return VIO_EINVAL;
    // ---- validation: nothing is written before all of it has passed
    if (h->hc.MX > 0 || h->hc.c.marg_exact) { g_err = "vio_debug_marg_set: the handle runs the literal marginalisation"; return VIO_EINVAL; }
    std::vector<char> live;
    VIO_TRY(stage_validate(h, in, "vio_debug_marg_set", false, live));
    return stage_write(h, seq, in, live, false);
}

int vio_debug_marg_run(vio_batch *h) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    VIO_TRY(vio_internal::launch_marg_all(h));
    return sync_all(h);
}

int vio_debug_marg_get(vio_batch *h, int seq, vio_marg_stage_out *out) {
    VIO_ENTER(h, seq, true);
    if (!out) return VIO_EINVAL;
    const DevCfg &C = h->hc;
    const Batch &B = h->B;
    const size_t W = C.W, n = C.NPRIOR, mq = 15 + n, s = (size_t)seq;
    std::vector<BeSeq> bev(1);
    const BeSeq &be = bev[0];
    HIPCHK(hipMemcpy(bev.data(), B.be + seq, sizeof(BeSeq), hipMemcpyDeviceToHost));
    if (out->prior_H) HIPCHK(hipMemcpy(out->prior_H, B.prior_H + s * n * n, n * n * sizeof(double), hipMemcpyDeviceToHost));
    if (out->prior_r) HIPCHK(hipMemcpy(out->prior_r, B.prior_r + s * n, n * sizeof(double), hipMemcpyDeviceToHost));
    if (out->prior_x0) HIPCHK(hipMemcpy(out->prior_x0, B.prior_x0 + s * (W * 7 + 17), (W * 7 + 17) * sizeof(double), hipMemcpyDeviceToHost));
    if (out->prior_present) for (size_t i = 0; i < W + 3; i++) out->prior_present[i] = be.prior_present[i];
    if (out->prior_c0) *out->prior_c0 = be.prior_c0;
    if (out->has_prior) *out->has_prior = be.has_prior;
    if (out->dbg5) for (int k = 0; k < 5; k++) out->dbg5[k] = be.dbg[k];
    const bool hbm = !h->marg_lds && C.MX == 0;
    if (out->hbm_valid) *out->hbm_valid = hbm ? 1 : 0;
    if (hbm) {
        if (out->margA) HIPCHK(hipMemcpy(out->margA, B.margA + s * mq * mq, mq * mq * sizeof(double), hipMemcpyDeviceToHost));
        if (out->margB) HIPCHK(hipMemcpy(out->margB, B.margB + s * mq, mq * sizeof(double), hipMemcpyDeviceToHost));
        if (out->margV) HIPCHK(hipMemcpy(out->margV, B.margV + s * n * n, n * n * sizeof(double), hipMemcpyDeviceToHost));
        if (out->b_r) HIPCHK(hipMemcpy(out->b_r, B.vec + s * VEC_SLOTS * C.LW, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return VIO_OK;
}

// ---- the solver on a staged state, launch by launch (include/vio_abi.h vio_debug_solve_set / _run / _get)
int vio_debug_solve_set(vio_batch *h, int seq, const vio_marg_stage_in *in) {
    VIO_ENTER(h, seq, true);
    if (!in) return VIO_EINVAL;
    std::vector<char> live;
    VIO_TRY(stage_validate(h, in, "vio_debug_solve_set", true, live));
    VIO_TRY(stage_write(h, seq, in, live, true));
    h->solve_staged.resize(h->S, 0);
    h->solve_staged[seq] = 1;
    return VIO_OK;
}

int vio_debug_solve_run(vio_batch *h, int slots, int stop_phase, double radius0) {
    VIO_ENTER(h, VIO_NO_SEQ, true);
    if (slots < 0) {
        if (stop_phase != VIO_SOLVE_STOP_NONE || radius0 != 0) { g_err = "vio_debug_solve_run: the whole solve takes no stop phase and no radius"; return VIO_EINVAL; }
        VIO_TRY(vio_internal::launch_solve_all(h, nullptr));
        return sync_all(h);
    }
    if (h->solve_mode != 1) { g_err = "vio_debug_solve_run: a handle without the phased solver runs the whole solve only (slots < 0)"; return VIO_EINVAL; }
    if (stop_phase < VIO_SOLVE_STOP_NONE || stop_phase > VIO_SOLVE_STOP_LS || !(radius0 >= 0) || !std::isfinite(radius0) ||
        slots + (stop_phase != VIO_SOLVE_STOP_NONE ? 1 : 0) > h->hc.c.max_iterations + h->extra_slots) {
        g_err = "vio_debug_solve_run: stop_phase, radius0 or the number of slots out of range";
        return VIO_EINVAL;
    }
    const vio_internal::SolveCut cut = {slots, stop_phase, radius0};   // (alive until sync_all has returned: its radius0 is copied asynchronously)
    VIO_TRY(vio_internal::launch_solve_all(h, &cut));
    return sync_all(h);
}

int vio_debug_solve_get(vio_batch *h, int seq, vio_solve_stage_out *out) {
    VIO_ENTER(h, seq, true);
    if (!out) return VIO_EINVAL;
    if (h->solve_mode != 1) { g_err = "vio_debug_solve_get: the handle does not run the phased solver"; return VIO_EINVAL; }
    const DevCfg &C = h->hc;
    const Batch &B = h->B;
    const size_t W1 = (size_t)C.W + 1, P = C.P, LW = C.LW, NL = C.NL, NLs = NL + 8, s = (size_t)seq, S = (size_t)B.S;
    std::vector<SolveSt> stv(1);
    const SolveSt &st = stv[0];
    HIPCHK(hipMemcpy(stv.data(), B.sst + seq, sizeof(SolveSt), hipMemcpyDeviceToHost));
    if (out->scal_i) {
        const int v[11] = {st.stage, st.iter, st.iters_done, st.F, st.Fa, st.nres, st.ex_active, st.td_active, st.vext, st.constrained, st.fused};
        for (int k = 0; k < 11; k++) out->scal_i[k] = v[k];
    }
    if (out->scal_d) {
        // ccost: ps_accept keeps the candidate's cost in a register (SolveSt::ccost is never written) and stores it as `cost` only when it accepts;
        // what it summed is still there: the partial costs of the last evaluation, one per workgroup or chunk, added here in index order
        const int nparts = std::min((int)PS_MAX_EVAL_BLOCKS, st.fused ? 2 + st.nblk : st.n_eval_blocks);
        double ccost = 0;
        for (int k = 0; k < nparts; k++) ccost += st.part[k];
        const double v[7] = {st.cost, ccost, st.radius, st.mu, st.alpha, st.dogleg_norm, st.model_change};
        for (int k = 0; k < 7; k++) out->scal_d[k] = v[k];
    }
    auto params = [&](const Params &X, double *o) {
        if (!o) return;
        memcpy(o, X.pose, 7 * W1 * sizeof(double)); memcpy(o + 7 * W1, X.sb, 9 * W1 * sizeof(double));
        memcpy(o + 16 * W1, X.ex, 7 * sizeof(double)); o[16 * W1 + 7] = X.td;
    };
    params(st.X, out->X); params(st.Xc, out->Xc);
    if (out->feat) HIPCHK(hipMemcpy(out->feat, B.para_feat + s * NL, NL * sizeof(double), hipMemcpyDeviceToHost));
    if (out->cfeat) HIPCHK(hipMemcpy(out->cfeat, B.cand_feat + s * NL, NL * sizeof(double), hipMemcpyDeviceToHost));
    // (the variable-landmark slots: the last NL entries of the sequence's pair_list, solve_prologue)
    if (out->var_slots) HIPCHK(hipMemcpy(out->var_slots, B.pair_list + s * C.NRES + C.NRES - NL, NL * sizeof(int), hipMemcpyDeviceToHost));
    if (out->H) {
        std::vector<double> Hd(LW * LW);
        HIPCHK(hipMemcpy(Hd.data(), B.H + s * LW * LW, LW * LW * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t a = 0; a < P; a++) memcpy(out->H + a * P, &Hd[a * LW], P * sizeof(double));
    }
    const double *vec = B.vec + s * VEC_SLOTS * LW, *lvec = B.lvec + s * NLs * 8;
    auto pvec = [&](double *o, int slot) { return o ? hipMemcpy(o, vec + slot * LW, P * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess; };
    auto lv = [&](double *o, const double *src) { return o ? hipMemcpy(o, src, NL * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess; };
    // (be_phased.h ps_serial_body: g, sp, dgp, gradp, gnp, stp = slots 0 .. 5 of c.vec; sl, dgl, gradl, gnl, stl = 0 .. 4 of c.lvec)
    HIPCHK(pvec(out->g, 0)); HIPCHK(pvec(out->sp, 1)); HIPCHK(pvec(out->dgp, 2)); HIPCHK(pvec(out->gnp, 4)); HIPCHK(pvec(out->stp, 5));
    HIPCHK(lv(out->sl, lvec)); HIPCHK(lv(out->dgl, lvec + NLs)); HIPCHK(lv(out->gnl, lvec + 3 * NLs)); HIPCHK(lv(out->stl, lvec + 4 * NLs));
    // the landmark rows of the current point: the half st.rowbuf of the double-buffered arrays (be_phased.h ps_sel_rows)
    const size_t rb = st.rowbuf ? 1 : 0;
    HIPCHK(lv(out->Hll, B.Hll + s * NLs + rb * S * NLs)); HIPCHK(lv(out->gl, B.gl + s * NLs + rb * S * NLs));
    if (out->Hpl) {
        std::vector<double> Wd(NL * LW);
        HIPCHK(hipMemcpy(Wd.data(), B.Hpl + s * NLs * LW + rb * S * NLs * LW, NL * LW * sizeof(double), hipMemcpyDeviceToHost));
        const size_t n0 = 6 * W1, e0 = 15 * W1, ne = st.vext ? 7 : 0;   // the columns the kernels write (ps_asm_a)
        for (size_t k = 0; k < NL; k++)
            for (size_t a = 0; a < P; a++) out->Hpl[k * P + a] = (a < n0 || (a >= e0 && a < e0 + ne)) ? Wd[k * LW + a] : 0.0;
    }
    if (out->Sc) {
        std::vector<double> Sd(LW * LW);
        HIPCHK(hipMemcpy(Sd.data(), B.Sc + s * LW * LW, LW * LW * sizeof(double), hipMemcpyDeviceToHost));
        const size_t nb = LW >> 4;
        for (size_t q = 0; q < LW * LW; q++) out->Sc[q] = 0.0;
        for (size_t ti = 0; ti < nb; ti++)
            for (size_t tj = 0; tj <= ti; tj++)
                for (size_t r = 0; r < 16; r++)
                    for (size_t c = 0; c < 16; c++)   // be_linalg.h tl_idx
                        out->Sc[(16 * ti + r) * LW + 16 * tj + c] = Sd[((ti * (ti + 1) / 2 + tj) << 8) + (r << 4) + (c ^ r)];
    }
    return VIO_OK;
}

int vio_stage_projection(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep, double td,
                         const double *obs_i, const double *obs_j, int use_td, double *r2, double *J46) {
    return stage_projection_impl(cfg, pose_i, pose_j, ex, inv_dep, td, obs_i, obs_j, use_td, 0, r2, J46);
}
int vio_stage_projection_residual(const vio_config *cfg, const double *pose_i, const double *pose_j, const double *ex, double inv_dep, double td,
                                  const double *obs_i, const double *obs_j, int use_td, double *r2, double *J46) {
    return stage_projection_impl(cfg, pose_i, pose_j, ex, inv_dep, td, obs_i, obs_j, use_td, 1, r2, J46);
}

int vio_stage_publish(int NL, int W, int n_lm, int ring_base, const vio_publish_tables *t, const int32_t *flags3, int cap, int32_t *counts4,
                      double *kf_pose8, double *cloud, double *margin, double *kf_points) {
    if (NL < 1 || W < 2 || W > VIO_MAXW || cap < 0 || !t || !flags3 || !counts4 || !kf_pose8) return VIO_EINVAL;
    if (!t->lm_order || !t->lm_id || !t->lm_start || !t->lm_nobs || !t->lm_solve_flag || !t->lm_dyn || !t->lm_depth || !t->lm_obs || !t->Ps ||
        !t->Rs || !t->Headers || !t->ric || !t->tic)
        return VIO_EINVAL;
    const size_t nl = (size_t)NL, W1 = (size_t)W + 1, c = (size_t)cap;
    // integers: the six tables, then counts; doubles: depth, observations, window, extrinsic, then the outputs (one more row each: cap may be 0)
    DevBuf<int> di;
    DevBuf<double> dd;
    const size_t o_cnt = 6 * nl;
    const size_t o_obs = nl, o_ps = o_obs + nl * W1 * VIO_OBS_D, o_rs = o_ps + 3 * W1, o_hd = o_rs + 9 * W1, o_ric = o_hd + W1, o_tic = o_ric + 9,
                 o_pose = o_tic + 3, o_cloud = o_pose + 8, o_margin = o_cloud + 3 * (c + 1), o_kf = o_margin + 3 * (c + 1), n_d = o_kf + 8 * (c + 1);
    HIPCHK(di.alloc(o_cnt + 4));
    HIPCHK(dd.alloc(n_d));
    const int32_t *tabs[6] = {t->lm_order, t->lm_id, t->lm_start, t->lm_nobs, t->lm_solve_flag, t->lm_dyn};
    for (int k = 0; k < 6; k++) HIPCHK(di.upload(tabs[k], nl, k * nl));
    HIPCHK(di.upload(counts4, 4, o_cnt));
    HIPCHK(dd.upload(t->lm_depth, nl));
    HIPCHK(dd.upload(t->lm_obs, nl * W1 * VIO_OBS_D, o_obs));
    HIPCHK(dd.upload(t->Ps, 3 * W1, o_ps));
    HIPCHK(dd.upload(t->Rs, 9 * W1, o_rs));
    HIPCHK(dd.upload(t->Headers, W1, o_hd));
    HIPCHK(dd.upload(t->ric, 9, o_ric));
    HIPCHK(dd.upload(t->tic, 3, o_tic));
    HIPCHK(dd.upload(kf_pose8, 8, o_pose));
    if (cloud && c) HIPCHK(dd.upload(cloud, 3 * c, o_cloud));
    if (margin && c) HIPCHK(dd.upload(margin, 3 * c, o_margin));
    if (kf_points && c) HIPCHK(dd.upload(kf_points, 8 * c, o_kf));
    // the row behind each list is a guard: a write at or beyond row `cap` fails the call
    const double guard[8] = {-1.5e300, -1.5e300, -1.5e300, -1.5e300, -1.5e300, -1.5e300, -1.5e300, -1.5e300};
    HIPCHK(dd.upload(guard, 3, o_cloud + 3 * c));
    HIPCHK(dd.upload(guard, 3, o_margin + 3 * c));
    HIPCHK(dd.upload(guard, 8, o_kf + 8 * c));
    PubIn in;
    in.lm_order = di; in.lm_id = di + nl; in.lm_start = di + 2 * nl; in.lm_nobs = di + 3 * nl; in.lm_solve_flag = di + 4 * nl; in.lm_dyn = di + 5 * nl;
    in.lm_depth = dd; in.lm_obs = dd + o_obs;
    in.n_lm = n_lm; in.NL = NL; in.W = W; in.ring_base = ring_base;
    in.Ps = dd + o_ps; in.Rs = dd + o_rs; in.Headers = dd + o_hd; in.ric = dd + o_ric; in.tic = dd + o_tic;
    in.solver_flag = flags3[0]; in.marginalization_flag = flags3[1]; in.processed = flags3[2];
    PubOut out;
    out.cap = cap; out.counts = di + o_cnt; out.kf_pose = dd + o_pose;
    out.cloud = cloud ? dd + o_cloud : nullptr; out.margin = margin ? dd + o_margin : nullptr; out.kf_points = kf_points ? dd + o_kf : nullptr;
    pub_stage_kernel<<<1, VIO_PUBLISH_BLOCK>>>(in, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(di.download(counts4, 4, o_cnt));
    HIPCHK(dd.download(kf_pose8, 8, o_pose));
    if (cloud && c) HIPCHK(dd.download(cloud, 3 * c, o_cloud));
    if (margin && c) HIPCHK(dd.download(margin, 3 * c, o_margin));
    if (kf_points && c) HIPCHK(dd.download(kf_points, 8 * c, o_kf));
    double back[14];
    HIPCHK(dd.download(back, 3, o_cloud + 3 * c));
    HIPCHK(dd.download(back + 3, 3, o_margin + 3 * c));
    HIPCHK(dd.download(back + 6, 8, o_kf + 8 * c));
    for (int k = 0; k < 14; k++)
        if (back[k] != guard[0]) { g_err = "vio_stage_publish: a row at or beyond cap was written"; return VIO_EDEVICE; }
    return VIO_OK;
}

}  // extern "C"
