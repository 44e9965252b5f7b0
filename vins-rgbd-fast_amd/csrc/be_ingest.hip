// be_ingest: the frame's features and IMU into the window (see be_ctx.h), with what only it calls -- the device solvePnP of VO mode,
// triangulateWithDepth, the IMU interval search -- and the two launches that share that code: be_preint_ahead_kernel (the next frame's IMU,
// off the chain) and be_dyn_finalize_kernel (hand-over of the host-side dynamic initialisation).  The stage kernels of the PnP, Rodrigues,
// extrinsic-calibration and pre-integration code live here too: pnp_refine_block, pnp_rodrigues*, ex_relative_r and preint_propagate* are not
// __forceinline__, so how many callers they have in this unit decides how they and their callers are compiled.
#include "be_ctx.h"
#include "be_linalg.h"
#include "be_excalib.h"
#include "be_preint.h"

// ------------------------------------------------------------------ VO mode: FeatureManager::initFramePoseByPnP
// cv::Rodrigues and its derivative (closed form, Gallego & Yezzi 2015), as the host side of the dynamic initialisation restates them
__device__ m3 pnp_rodrigues(v3 r) {
    const double th = nrm(r);
    if (th < 2.220446049250313e-16) return eye();
    const v3 k = scl(1.0 / th, r);
    const double cth = cos(th), sth = sin(th), c1 = 1 - cth;
    const m3 K = skew(k);
    const double kk[3] = {k.x, k.y, k.z};
    m3 R;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.a[i * 3 + j] = (i == j ? cth : 0.0) + c1 * kk[i] * kk[j] + sth * K.a[i * 3 + j];
    return R;
}
__device__ v3 pnp_rodrigues_inv(const m3 &R) {
    v3 r = mk(R.a[7] - R.a[5], R.a[2] - R.a[6], R.a[3] - R.a[1]);
    const double sn = sqrt(dot(r, r) * 0.25);
    double cs = (R.a[0] + R.a[4] + R.a[8] - 1) * 0.5;
    cs = cs > 1 ? 1 : (cs < -1 ? -1 : cs);
    const double th = acos(cs);
    if (sn < 1e-5) {
        if (cs > 0) return mk(0, 0, 0);
        v3 v;
        v.x = sqrt(fmax((R.a[0] + 1) * 0.5, 0.0));
        v.y = sqrt(fmax((R.a[4] + 1) * 0.5, 0.0)) * (R.a[1] < 0 ? -1.0 : 1.0);
        v.z = sqrt(fmax((R.a[8] + 1) * 0.5, 0.0)) * (R.a[2] < 0 ? -1.0 : 1.0);
        if (fabs(v.x) < fabs(v.y) && fabs(v.x) < fabs(v.z) && (R.a[5] > 0) != (v.y * v.z > 0)) v.z = -v.z;
        return scl(th / nrm(v), v);
    }
    return scl(th / (2 * sn), r);
}
// dR / dr_i (i = 0 .. 2) at r, Rm = pnp_rodrigues(r)
__device__ void pnp_rodrigues_jac(v3 r, const m3 &Rm, m3 dR[3]) {
    const double th2 = dot(r, r);
    for (int i = 0; i < 3; i++) {
        const v3 e = mk(i == 0, i == 1, i == 2);
        if (th2 < 1e-24) { dR[i] = skew(e); continue; }
        const v3 w = cross(r, mul(sub(eye(), Rm), e));
        dR[i] = scl(1.0 / th2, mul(add(scl(get(r, i), skew(r)), skew(w)), Rm));
    }
}
// The Levenberg-Marquardt core of cv::solvePnP(ITERATIVE): refines par[6] = (rvec, tvec) in LDS over n pairs pts[5 n] = (X, Y, Z, u, v).
// prev: 6 doubles of LDS, sw: >= (waves x 28) doubles of LDS.  Every thread of the block takes part.  trace (may be null, written by thread
// 0): outer iterations, lambda escalations, final lambda_lg10.
__device__ void pnp_refine_block(const double *pts, int n, double *sh_par, double *sh_prev, double *sw, int *trace = nullptr) {
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    // reduction of NV values per thread: wave DPP sums, then a fixed-order sum over the waves
    auto reduce = [&](double *v, int NV) {
        for (int q = 0; q < NV; q++) v[q] = wave_sum_dpp(v[q]);
        __syncthreads();
        if (lane == 0) for (int q = 0; q < NV; q++) sw[wave * 28 + q] = v[q];
        __syncthreads();
        for (int q = 0; q < NV; q++) { double r = 0; for (int w = 0; w < nw; w++) r += sw[w * 28 + q]; v[q] = r; }
    };
    // residuals (and Jacobian sums) at sh_par; every thread returns the same values
    auto project = [&](bool jac, double *acc /*27: JtJ upper 21 + JtErr 6*/) -> double {
        const v3 r = mk(sh_par[0], sh_par[1], sh_par[2]), tt = mk(sh_par[3], sh_par[4], sh_par[5]);
        const m3 Rm = pnp_rodrigues(r);
        m3 dR[3];
        if (jac) pnp_rodrigues_jac(r, Rm, dR);
        double v[28];
        for (int q = 0; q < 28; q++) v[q] = 0;
        for (int i = t; i < n; i += nt) {
            const double *q = pts + (size_t)i * 5;
            const v3 Y = add(mul(Rm, mk(q[0], q[1], q[2])), tt);
            const double iz = 1.0 / Y.z, x = Y.x * iz, y = Y.y * iz;
            const double e0 = x - q[3], e1 = y - q[4];
            v[27] += e0 * e0 + e1 * e1;
            if (!jac) continue;
            double J0[6], J1[6];
            for (int k = 0; k < 3; k++) {
                const v3 d = mul(dR[k], mk(q[0], q[1], q[2]));
                J0[k] = iz * d.x - x * iz * d.z;
                J1[k] = iz * d.y - y * iz * d.z;
            }
            J0[3] = iz; J0[4] = 0; J0[5] = -x * iz;
            J1[3] = 0; J1[4] = iz; J1[5] = -y * iz;
            int e = 0;
            for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) v[e++] += J0[a] * J0[b] + J1[a] * J1[b];
            for (int a = 0; a < 6; a++) v[21 + a] += J0[a] * e0 + J1[a] * e1;
        }
        reduce(v, jac ? 28 : 28);
        if (jac) for (int q = 0; q < 27; q++) acc[q] = v[q];
        return sqrt(v[27]);
    };
    double acc[27];
    int lambda_lg10 = -3, iters = 0, raises = 0;
    double prev_err = 0;
    auto take_step = [&]() {   // thread 0: param = prev - pinv(JtJ with damped diagonal) JtErr
        if (t == 0) {
            const double lambda = exp(lambda_lg10 * 2.302585092994046);
            double N[36], V[36];
            int e = 0;
            for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { N[a * 6 + b] = acc[e]; N[b * 6 + a] = acc[e]; e++; }
            for (int a = 0; a < 6; a++) N[a * 7] *= 1.0 + lambda;
            jacobi_small(N, V, 6);
            double wmax = 0;
            for (int k = 0; k < 6; k++) wmax = fmax(wmax, fabs(N[k * 7]));
            double d[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 6; k++) {
                const double wk = N[k * 7];
                if (!(fabs(wk) > wmax * 2 * 2.220446049250313e-16 * 6)) continue;
                double sacc = 0;
                for (int i = 0; i < 6; i++) sacc += V[i * 6 + k] * acc[21 + i];
                sacc /= wk;
                for (int i = 0; i < 6; i++) d[i] += V[i * 6 + k] * sacc;
            }
            for (int i = 0; i < 6; i++) sh_par[i] = sh_prev[i] - d[i];
        }
        __syncthreads();
    };
    for (;;) {
        const double e_at = project(true, acc);
        if (t == 0) for (int i = 0; i < 6; i++) sh_prev[i] = sh_par[i];
        __syncthreads();
        take_step();
        if (iters == 0) prev_err = e_at;
        bool done = false;
        for (;;) {
            const double e = project(false, acc);
            if (e > prev_err && ++lambda_lg10 <= 16) { raises++; take_step(); continue; }
            lambda_lg10 = max(lambda_lg10 - 1, -16);
            double dn = 0, pn = 0;
            for (int i = 0; i < 6; i++) { dn += (sh_par[i] - sh_prev[i]) * (sh_par[i] - sh_prev[i]); pn += sh_prev[i] * sh_prev[i]; }
            // cvNorm(param, prevParam, CV_RELATIVE_L2) = |param - prev| / (|prev| + DBL_EPSILON)
            if (++iters >= 20 || sqrt(dn) / (sqrt(pn) + 2.220446049250313e-16) < 1.1920928955078125e-07) done = true;
            prev_err = e;
            break;
        }
        if (done) break;
    }
    if (trace && t == 0) { trace[0] = iters; trace[1] = raises; trace[2] = lambda_lg10; }
    __syncthreads();
}

// FeatureManager::initFramePoseByPnP + solvePoseByPnP (feature_manager.cpp:545-642): cv::solvePnP(SOLVEPNP_ITERATIVE,
// useExtrinsicGuess) = CvLevMarq on (rvec, tvec) with lambda = 10^k, diagonal x (1 + lambda), at most 20 iterations, FLT_EPSILON
// on the relative parameter change.  Block-cooperative: one thread per 3-D / 2-D pair evaluates its two residual rows and 2 x 6
// Jacobian, the 27 sums of J^T J / J^T e are reduced in a fixed order, thread 0 solves the damped 6 x 6 system through its
// eigen-decomposition (cv::solve DECOMP_SVD).  pts: scratch in HBM, 5 doubles per pair.  sw: >= 16 * 28 + 64 doubles of LDS.
__device__ void init_frame_pose_by_pnp(Ctx &c, int fc, double *pts, double *sw) {
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    BeSeq &be = *c.be;
    if (fc <= 0) return;
    __shared__ int sh_n;
    __shared__ double sh_par[6], sh_prev[6], sh_flag[4];
    if (t == 0) sh_n = 0;
    __syncthreads();
    const m3 ric = ldm(be.ric);
    const v3 tic = ld3(be.tic);
    const int nlm = be.n_lm;
    // pairs in list order (deterministic): flags + scan
    int *flag = c.lm_pidx, *offs = c.lm_aidx;   // free outside the solve
    __shared__ int scan_scratch[2 * 256 + 8];
    for (int k = t; k < nlm; k += nt) {
        const int slot = c.lm_order[k];
        const int index = fc - c.lm_start[slot];
        flag[k] = (c.lm_depth[slot] > 0 && index >= 0 && c.lm_nobs[slot] >= index + 1) ? 1 : 0;
    }
    __syncthreads();
    const int n = block_scan_flags(flag, nlm, offs, scan_scratch);
    for (int k = t; k < nlm; k += nt) {
        if (!flag[k]) continue;
        const int slot = c.lm_order[k], st = c.lm_start[slot];
        const double *o0 = obs_ptr(c, slot, st), *oi = obs_ptr(c, slot, fc);
        const double d = c.lm_depth[slot];
        const v3 pc = add(mul(ric, mk(o0[0] * d, o0[1] * d, o0[2] * d)), tic);
        const v3 pw = add(mul(ldm(be.Rs[st]), pc), ld3(be.Ps[st]));
        double *q = pts + (size_t)offs[k] * 5;
        q[0] = (double)(float)pw.x; q[1] = (double)(float)pw.y; q[2] = (double)(float)pw.z;   // cv::Point3f / cv::Point2f
        q[3] = (double)(float)oi[0]; q[4] = (double)(float)oi[1];
    }
    __syncthreads();
    if (n < 4) return;
    if (t == 0) {
        const m3 RCam = mul(ldm(be.Rs[fc - 1]), ric);
        const v3 PCam = add(mul(ldm(be.Rs[fc - 1]), tic), ld3(be.Ps[fc - 1]));
        const m3 R0 = tr(RCam);
        const v3 P0 = neg(mul(R0, PCam));
        const v3 r = pnp_rodrigues_inv(R0);
        sh_par[0] = r.x; sh_par[1] = r.y; sh_par[2] = r.z; sh_par[3] = P0.x; sh_par[4] = P0.y; sh_par[5] = P0.z;
    }
    __syncthreads();
    pnp_refine_block(pts, n, sh_par, sh_prev, sw);
    __syncthreads();
    if (t == 0) {
        bool fin = true;
        for (int i = 0; i < 6; i++) fin = fin && isfinite(sh_par[i]);
        if (fin) {
            const m3 Rn = pnp_rodrigues(mk(sh_par[0], sh_par[1], sh_par[2]));
            const v3 tn = mk(sh_par[3], sh_par[4], sh_par[5]);
            const m3 RCam = tr(Rn);
            const v3 PCam = mul(RCam, neg(tn));
            stm(be.Rs[fc], mul(RCam, tr(ric)));
            st3(be.Ps[fc], add(neg(mul(RCam, mul(tr(ric), tic))), PCam));
        }
    }
    __syncthreads();
}

// FeatureManager::triangulateWithDepth (feature_manager.cpp:386-543), one thread per landmark of the list
__device__ void triangulate_with_depth(Ctx &c, int nlm) {
    const int t = threadIdx.x, nt = blockDim.x;
    BeSeq &be = *c.be;
    const vio_config &cfg = c.C->c;
        m3 ric = ldm(be.ric);
        v3 tic = ld3(be.tic);
        for (int k = t; k < nlm; k += nt) {
            int slot = c.lm_order[k];
            if (c.lm_depth[slot] > 0) continue;
            if (!in_problem(c, slot)) continue;
            int imu_i = c.lm_start[slot], K = c.lm_nobs[slot];
            v3 trr = add(ld3(be.Ps[imu_i]), mul(ldm(be.Rs[imu_i]), tic));
            m3 Rr = mul(ldm(be.Rs[imu_i]), ric);
            double vsum = 0, rsum = 0;
            int vn = 0, rn = 0, no_depth = 0;
            for (int a = 0; a < K; a++) {
                const double *oa = obs_ptr(c, slot, imu_i + a);
                if (oa[8] == 0) { no_depth++; continue; }
                v3 t0 = add(ld3(be.Ps[imu_i + a]), mul(ldm(be.Rs[imu_i + a]), tic));
                m3 R0 = mul(ldm(be.Rs[imu_i + a]), ric);
                v3 point0 = scl(oa[8], mk(oa[0], oa[1], oa[2]));
                point0 = mk(oa[0] * oa[8], oa[1] * oa[8], oa[2] * oa[8]);
                v3 t2r = mul(tr(Rr), sub(t0, trr));
                m3 R2r = mul(tr(Rr), R0);
                for (int b = 0; b < K; b++) {
                    if (a == b) continue;
                    const double *ob = obs_ptr(c, slot, imu_i + b);
                    v3 t1 = add(ld3(be.Ps[imu_i + b]), mul(ldm(be.Rs[imu_i + b]), tic));
                    m3 R1 = mul(ldm(be.Rs[imu_i + b]), ric);
                    v3 t20 = mul(tr(R0), sub(t1, t0));
                    m3 R20 = mul(tr(R0), R1);
                    v3 pp = sub(mul(tr(R20), point0), mul(tr(R20), t20));
                    double rx = ob[0] - pp.x / pp.z, ry = ob[1] - pp.y / pp.z;
                    if (sqrt(rx * rx + ry * ry) < 10.0 / 460) {
                        v3 pr = add(mul(R2r, point0), t2r);
                        if (oa[8] > cfg.depth_max) { rsum += pr.z; rn++; } else { vsum += pr.z; vn++; }
                    }
                }
            }
            double dep;
            int ef;
            if (vn == 0) {
                if (rn == 0) {
                    if (no_depth == K) {
                        double AtA[16], Vv[16];
                        for (int q = 0; q < 16; q++) AtA[q] = 0;
                        v3 t0 = add(ld3(be.Ps[imu_i]), mul(ldm(be.Rs[imu_i]), tic));
                        m3 R0 = mul(ldm(be.Rs[imu_i]), ric);
                        for (int a = 0; a < K; a++) {
                            const double *oa = obs_ptr(c, slot, imu_i + a);
                            v3 t1 = add(ld3(be.Ps[imu_i + a]), mul(ldm(be.Rs[imu_i + a]), tic));
                            m3 R1 = mul(ldm(be.Rs[imu_i + a]), ric);
                            v3 tt = mul(tr(R0), sub(t1, t0));
                            m3 Rt = tr(mul(tr(R0), R1));
                            v3 mt = neg(mul(Rt, tt));
                            double Pm[12];
                            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) Pm[r * 4 + q] = Rt.a[r * 3 + q]; Pm[r * 4 + 3] = get(mt, r); }
                            v3 f = mk(oa[0], oa[1], oa[2]);
                            f = scl(1.0 / nrm(f), f);
                            f = mk(oa[0] / nrm(mk(oa[0], oa[1], oa[2])), oa[1] / nrm(mk(oa[0], oa[1], oa[2])), oa[2] / nrm(mk(oa[0], oa[1], oa[2])));
                            double row[8];
                            for (int q = 0; q < 4; q++) { row[q] = f.x * Pm[8 + q] - f.z * Pm[q]; row[4 + q] = f.y * Pm[8 + q] - f.z * Pm[4 + q]; }
                            for (int rr = 0; rr < 2; rr++)
                                for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) AtA[x * 4 + y] += row[rr * 4 + x] * row[rr * 4 + y];
                        }
                        jacobi_small(AtA, Vv, 4);
                        int mi = 0;
                        for (int q = 1; q < 4; q++) if (AtA[q * 5] < AtA[mi * 5]) mi = q;
                        double svd_method = Vv[2 * 4 + mi] / Vv[3 * 4 + mi];
                        dep = svd_method < cfg.depth_min ? cfg.depth_max : svd_method;
                        ef = 2;
                    } else
                        continue;
                } else { dep = rsum / rn; ef = 0; }
            } else { dep = vsum / vn; ef = 1; }
            if (dep < 0.1) { dep = cfg.init_depth; ef = 0; }
            c.lm_depth[slot] = dep;
            c.lm_est[slot] = ef;
        }
}

// ====================================================================================================== the frame's IMU, ahead of be_ingest
// getIMUInterval (estimator.cpp:1910-1942) on a sequence's ring, by one wavefront: head = the first sample later than prevT from head0 on, k = the
// first one at or after curTime: 64 samples per trip, one lane each (the two scalar loops were a chain of dependent loads, ~14 of them per frame at
// 200 Hz).  Every lane returns the same head and k.
__device__ __forceinline__ void imu_interval_search(const double *it, int NIMU, int cnt_all, double prevT, double curTime, int head0, int &head, int &k) {
    const int t = threadIdx.x & 63;
    head = head0;
    for (;;) {
        const int idx = head + t;
        const bool pass = idx < cnt_all && it[idx % NIMU] <= prevT;
        const unsigned long long stop = ~__ballot(pass);
        if (stop) { head += __ffsll((long long)stop) - 1; break; }
        head += 64;
    }
    k = head;
    for (;;) {
        const int idx = k + t;
        const bool pass = idx < cnt_all && it[idx % NIMU] < curTime;
        const unsigned long long stop = ~__ballot(pass);
        if (stop) { k += __ffsll((long long)stop) - 1; break; }
        k += 64;
    }
}
// PreAhead::in, entry i, as the sequence holds it now
__device__ __forceinline__ const double *ahead_in_ptr(const BeSeq &be, int W, int i) {
    return i < 3 ? be.acc_0 + i : i < 6 ? be.gyr_0 + (i - 3) : i < 9 ? be.Ps[W] + (i - 6) : i < 12 ? be.Vs[W] + (i - 9) : i < 21 ? be.Rs[W] + (i - 12)
         : i < 24 ? be.Bas[W] + (i - 21) : i < 27 ? be.Bgs[W] + (i - 24) : be.g + (i - 27);
}
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// What be_ingest does between its feature part and the triangulation for a steady-state frame (NON_LINEAR, full window), on copies: the interval search,
// the fresh pre-integration of slot W and its n propagate steps with processIMU's world-state recursion as the side job -- through the very device
// functions be_ingest calls, so that the bits are the same.  Its inputs are final once the previous frame's solve has ended (the window slide of
// be_marg never writes slot W of Ps / Vs / Rs / Bas / Bgs, nor acc_0 / gyr_0 / g / td / prevTime / imu_head), so it runs beside that frame's be_marg.
// It reads the sequence and writes nothing but its record.
__global__ __launch_bounds__(256) void be_preint_ahead_kernel(Batch B, const double *stamps, PreAhead *ahead) {
    const int s = blockIdx.x + B.s0, t = threadIdx.x;
    Ctx c = make_ctx(B, s);
    const DevCfg &C = *B.cfg;
    const vio_calibration &K = *c.K;
    const BeSeq &be = *c.be;
    const int W = c.W;
    PreAhead &rec = ahead[s];
    __shared__ int sh_i[8];
    __shared__ double sh_in[30];
    __shared__ PreWork pw;
    __shared__ double pi_fv[PREINT_MANY_LDS_DOUBLES];
    const double *it = B.imu_t + (size_t)s * C.NIMU;
    const double *ia = B.imu_acc + (size_t)s * C.NIMU * 3, *ig = B.imu_gyr + (size_t)s * C.NIMU * 3;
    const double stamp = stamps[s], prevT = be.prevTime, curTime = stamp + be.td;
    const int head0 = be.imu_head, cnt_all = be.imu_count;
    if (t < 30) sh_in[t] = *ahead_in_ptr(be, W, t);
    if (t == 0) {
        bool ok = C.c.use_imu && W > 0 && be.solver_flag == 1 && be.frame_count == W && !be.rebooted && be.first_imu && be.initFirstPoseFlag;
        ok = ok && head0 >= 0 && cnt_all > head0 && cnt_all - head0 <= C.NIMU;   // (a longer backlog: be_ingest moves the head and flags the overrun)
        ok = ok && curTime <= it[(cnt_all - 1) % C.NIMU];                          // the IMU reaches the frame (estimator.cpp:178-183)
        sh_i[0] = ok;
        if (!ok) rec.valid = 0;
    }
    __syncthreads();
    if (!sh_i[0]) return;
    if (t < 64) {
        int head, k;
        imu_interval_search(it, C.NIMU, cnt_all, prevT, curTime, head0, head, k);
        sh_i[6] = head; sh_i[7] = k;
    }
    PreInt &P = rec.pre;
    if (t == 0) {
        rec.valid = 0;   // until the record is complete
        rec.stamp = stamp; rec.cur_time = curTime; rec.prev_time = prevT;
        rec.imu_head = head0; rec.imu_count = cnt_all;
        rec.noise[0] = K.acc_n; rec.noise[1] = K.gyr_n; rec.noise[2] = K.acc_w; rec.noise[3] = K.gyr_w;
        bf::preint_init(P, ld3(sh_in), ld3(sh_in + 3), ld3(sh_in + 21), ld3(sh_in + 24));
    }
    if (t >= 64 && t < 94) rec.in[t - 64] = sh_in[t - 64];
    __syncthreads();
    const int head = sh_i[6], n = sh_i[7] - head + 1;
    preint_load(P, pw);
    const PreintRing ring = {it, ia, ig, head, C.NIMU, prevT, curTime, n};
    WorldStep ws = {ld3(sh_in), ld3(sh_in + 3), ld3(sh_in + 6), ld3(sh_in + 9), ldm(sh_in + 12), ld3(sh_in + 21), ld3(sh_in + 24), ld3(sh_in + 27)};
    preint_propagate_many<true>(P, pw, K, n, ring, ws, true, pi_fv);
    if (t == 64) { st3(rec.out, ws.P); st3(rec.out + 3, ws.V); stm(rec.out + 6, ws.R); st3(rec.out + 15, ws.a0); st3(rec.out + 18, ws.g0); }
    preint_store(P, pw);
    if (t == 0) { rec.head = head; rec.k = sh_i[7]; rec.n = n; rec.valid = 1; }
}

// be_ingest's side: is `rec` the result of exactly the integration this frame would run (every input bit for bit, slot W's pre-integration P the
// untouched fresh one)?  Then file it -- what the integration would have written, no byte more (the tails of the slot's sample buffers keep their stale
// content, as they do today) -- and return true.  Every thread of the block, uniform result.
__device__ __forceinline__ bool preint_ahead_take(Ctx &c, PreAhead &rec, double stamp, double curTime, int *sh_flag) {
    const int t = threadIdx.x, nt = blockDim.x, W = c.W;
    BeSeq &be = *c.be;
    const vio_calibration &K = *c.K;
    PreInt &P = c.pre[be.pre_idx[W]];
    if (t < 64) {
        bool ok = true;
        if (t < 30) ok = same_bits(rec.in[t], *ahead_in_ptr(be, W, t));
        else if (t < 42) { const int i = t - 30; ok = same_bits(P.lin_acc[i], rec.in[i < 6 ? i : i + 15]); }   // lin_acc lin_gyr lin_ba lin_bg, contiguous
        else if (t == 42) ok = same_bits(rec.noise[0], K.acc_n) && same_bits(rec.noise[1], K.gyr_n) && same_bits(rec.noise[2], K.acc_w) && same_bits(rec.noise[3], K.gyr_w);
        else if (t == 43) ok = same_bits(rec.stamp, stamp) && same_bits(rec.cur_time, curTime) && same_bits(rec.prev_time, be.prevTime);
        else if (t == 44) ok = rec.valid == 1 && rec.imu_head == be.imu_head && rec.imu_count == be.imu_count && P.valid && P.n_buf == 0 && be.first_imu && be.initFirstPoseFlag;
        const bool all = __ballot(ok) == ~0ull;
        if (t == 0) *sh_flag = all;
    }
    __syncthreads();
    if (!*sh_flag) return false;
    const int n = rec.n, m = min(n, VIO_IMU_SLOT_CAP);
    const PreInt &Q = rec.pre;
    {
        double *d = (double *)&P;
        const double *q = (const double *)&Q;
        for (int i = t; i < (int)(offsetof(PreInt, dt_buf) / sizeof(double)); i += nt) d[i] = q[i];
        for (int i = t; i < m; i += nt) P.dt_buf[i] = Q.dt_buf[i];
        for (int i = t; i < 3 * m; i += nt) { (&P.acc_buf[0][0])[i] = (&Q.acc_buf[0][0])[i]; (&P.gyr_buf[0][0])[i] = (&Q.gyr_buf[0][0])[i]; }
    }
    if (t >= 64 && t < 85) {
        const int i = t - 64;
        double *d = i < 3 ? be.Ps[W] + i : i < 6 ? be.Vs[W] + (i - 3) : i < 15 ? be.Rs[W] + (i - 6) : i < 18 ? be.acc_0 + (i - 15) : be.gyr_0 + (i - 18);
        *d = rec.out[i];
    }
    if (t == 0) {
        P.n_buf = Q.n_buf;
        be.imu_head = rec.k;   // that last sample is not popped
        be.n_imu_frame = n;
        be.imu_frame_head = rec.head;
        be.prevTime = curTime;
        if (n > VIO_IMU_SLOT_CAP) be.overflow |= 2;
        rec.used++;
    }
    __syncthreads();
    return true;
}

// ====================================================================================================== be_ingest
// src.ids == NULL: the feature map packaged by the last vio_track / front-end of vio_feed (B.obs_id / B.obs / FeSeq);
// otherwise a caller-supplied map (vio_process_obs = Estimator::processImage(image, header), estimator.h:46): n_obs[s] < 0 skips s.
// EXCALIB (estimate_extrinsic = 2 handles only): the extrinsic-rotation calibration phase (be_excalib.h) runs after the pre-integration; the
// dynamic LDS then also holds the correspondences (4 NP doubles, see vio_abi.hip ingest_lds_bytes).
template <bool EXCALIB>
__global__ __launch_bounds__(256) void be_ingest_kernel(Batch B, const uint16_t *depth_base, size_t depth_stride, IngestSrc src) {
    const int s = blockIdx.x + B.s0, t = threadIdx.x, nt = blockDim.x;
    Ctx c = make_ctx(B, s);
    const DevCfg &C = *B.cfg;
    const vio_config &cfg = C.c;
    const vio_calibration &K = *c.K;   // the sequence's IMU noise
    BeSeq &be = *c.be;
    FeSeq &fe = *c.fe;
    const int W = c.W;
    __shared__ int sh_i[8];
    __shared__ double sh_d[8];
    __shared__ int scratch[2 * 256 + 8];
    __shared__ double sred[256];
    __shared__ PreWork pw;
    PH_INIT;
    const bool ext = src.ids != nullptr;
    const int ext_n = ext ? src.n_obs[s] : 0;
    const double in_stamp = ext ? src.stamps[s] : fe.cur_time;
    if (t == 0) {
        // the state the next call's tracker sees with tracker lag 1 (that tracker runs while THIS frame is still being optimised)
        for (int k = 0; k < 3; k++) be.track_Bg[k] = be.latest_Bg[k];
        be.track_td = be.td;
        be.imu_count_ingest = be.imu_count;
        be.do_solve = 0; be.do_marg = 0; be.processed = 0; be.rebooted = 0; be.init_frame = 0; be.dyn_failed = 0;
        be.status_code = (!ext && fe.n_forw == -2) ? VIO_NEED_IMU : VIO_OK;
        be.cur_stamp = in_stamp;
        be.overflow = 0;
        if (be.imu_count - be.imu_head > C.NIMU) { be.imu_head = be.imu_count - C.NIMU; be.overflow |= 16; }  // samples overwritten in the ring before they were consumed
    }
    __syncthreads();
    PreAhead *const ahead = src.ahead ? src.ahead + s : nullptr;   // a record that is not taken over counts as declined, whatever the reason
    if (ext ? ext_n <= 0 : (fe.n_forw < 0 || !fe.publish_ok)) {
        if (ahead && t == 0) ahead->declined++;
        return;
    }
    // ---- IMU availability (estimator.cpp:178-183, :1882-1888)
    const double *it = B.imu_t + (size_t)s * C.NIMU;
    const double *ia = B.imu_acc + (size_t)s * C.NIMU * 3, *ig = B.imu_gyr + (size_t)s * C.NIMU * 3;
    double stamp = in_stamp, curTime = stamp + be.td;
    if (cfg.use_imu) {
        bool have = be.imu_count > be.imu_head;
        double back_t = have ? it[(be.imu_count - 1) % C.NIMU] : -1e300;
        if (!(have && curTime <= back_t)) {
            if (t == 0) { be.status_code = VIO_NEED_IMU; if (ahead) ahead->declined++; }
            return;
        }
    }
    const uint16_t *depth = depth_base + (size_t)s * depth_stride;
    const int fc = be.frame_count;
    // ---- addFeatureCheckParallax (feature_manager.cpp:56-123)
    int nobs = ext ? min(ext_n, C.NP) : fe.n_obs, nlm = be.n_lm;
    const int *o_id = ext ? src.ids + (size_t)s * src.cap : B.obs_id + (size_t)s * C.NP;
    const double *o = ext ? src.obs + (size_t)s * src.cap * 7 : B.obs + (size_t)s * C.NP * 7;
    int *flag = c.lm_tmp;         // new-landmark flags per observation (NP <= NL is checked at create)
    int *offs = c.lm_pidx;        // temporary
    int tracked = 0;
    // id -> slot lookup (feature_manager.cpp:66-67 find_if over the list).  The list is NOT sorted by id: a landmark removed by
    // outlier rejection while the tracker keeps its id is re-appended at the end.  Open-addressing hash table in LDS.
    extern __shared__ int htab[];  // [2 * HT]: keys, values
    const int HT = C.lm_hash_size;
    for (int q = t; q < HT; q += nt) htab[q] = -1;
    __syncthreads();
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k], id = c.lm_id[slot];
        unsigned hsh = ((unsigned)id * 2654435761u) & (unsigned)(HT - 1);
        while (atomicCAS(&htab[hsh], -1, id) != -1) hsh = (hsh + 1) & (unsigned)(HT - 1);
        htab[HT + hsh] = slot;
    }
    __syncthreads();
    for (int j = t; j < nobs; j += nt) {
        const double *p = o + (size_t)j * 7;
        unsigned short mm = depth[(size_t)min(max((int)p[4], 0), cfg.height - 1) * cfg.width + min(max((int)p[3], 0), cfg.width - 1)];
        double dmm = mm / 1000.0;
        int isnew = 0;
        if (!(0 < dmm && dmm < cfg.depth_min)) {
            int fid = o_id[j];
            int found = -1;
            unsigned hsh = ((unsigned)fid * 2654435761u) & (unsigned)(HT - 1);
            while (htab[hsh] != -1) {
                if (htab[hsh] == fid) { found = htab[HT + hsh]; break; }
                hsh = (hsh + 1) & (unsigned)(HT - 1);
            }
            if (found >= 0) {
                int k = c.lm_nobs[found];
                if (k <= W) {
                    double *q = obs_ptr(c, found, c.lm_start[found] + k);
                    for (int d = 0; d < 7; d++) q[d] = p[d];
                    q[7] = be.td; q[8] = dmm;
                    c.lm_nobs[found] = k + 1;
                }
                tracked++;
            } else
                isnew = 1;
        }
        flag[j] = isnew;
    }
    __syncthreads();
    PH(106);
    {
        double tr = block_sum((double)tracked, sred);
        if (t == 0) be.last_track_num = (int)tr;
    }
    int nnew = block_scan_flags(flag, nobs, offs, scratch);
    {
        int nfree = be.n_free;
        int can = min(nnew, nfree);
        for (int j = t; j < nobs; j += nt) {
            if (!flag[j] || offs[j] >= can) continue;
            int slot = c.lm_free[nfree - 1 - offs[j]];
            const double *p = o + (size_t)j * 7;
            unsigned short mm = depth[(size_t)min(max((int)p[4], 0), cfg.height - 1) * cfg.width + min(max((int)p[3], 0), cfg.width - 1)];
            c.lm_id[slot] = o_id[j]; c.lm_start[slot] = fc; c.lm_nobs[slot] = 1; c.lm_est[slot] = 0; c.lm_solve[slot] = 0;
            c.lm_dyn[slot] = 0; c.lm_depth[slot] = -1.0;
            double *q = obs_ptr(c, slot, fc);
            for (int d = 0; d < 7; d++) q[d] = p[d];
            q[7] = be.td; q[8] = mm / 1000.0;
            c.lm_order[nlm + offs[j]] = slot;
        }
        __syncthreads();
        if (t == 0) {
            be.n_lm = nlm + can; be.n_free = nfree - can;
            if (can < nnew) be.overflow |= 1;
        }
        __syncthreads();
        nlm = be.n_lm;
    }
    PH(107);
    // parallax (:100-122, :732-768)
    {
        double psum = 0, pnum = 0;
        if (!(fc < 2 || be.last_track_num < 20)) {
            for (int k = t; k < nlm; k += nt) {
                int slot = c.lm_order[k];
                int st = c.lm_start[slot], no = c.lm_nobs[slot];
                if (st <= fc - 2 && st + no - 1 >= fc - 1) {
                    const double *fi = obs_ptr(c, slot, fc - 2), *fj = obs_ptr(c, slot, fc - 1);
                    double dep_i = fi[2], u_i = fi[0] / dep_i, v_i = fi[1] / dep_i;
                    double du = u_i - fj[0], dv = v_i - fj[1];
                    psum += fmax(0.0, sqrt(fmin(du * du + dv * dv, du * du + dv * dv)));
                    pnum += 1.0;
                }
            }
        }
        psum = block_sum(psum, sred);
        pnum = block_sum(pnum, sred);
        if (t == 0) {
            bool kf;
            if (fc < 2 || be.last_track_num < 20) kf = true;
            else if (pnum == 0) kf = true;
            else kf = psum / pnum >= cfg.min_parallax_px / cfg.focal_length;
            be.marginalization_flag = kf ? 0 : 1;
            be.Headers[fc] = stamp;
        }
        __syncthreads();
    }
    PH(108);
    // ---- getIMUInterval + processIMU (estimator.cpp:185-200, 1910-1942, 118-154); VO mode (USE_IMU == 0) has neither.  A steady-state frame whose
    // interval be_preint_ahead_kernel has integrated already, from exactly these inputs, only files that result.
    bool imu_here = cfg.use_imu;
    if (ahead && imu_here) {
        if (fc == W && fc != 0 && preint_ahead_take(c, *ahead, stamp, curTime, &sh_i[5])) imu_here = false;
        else if (t == 0) ahead->declined++;
    }
    if (imu_here && t < 64) {
        int head, k;
        imu_interval_search(it, C.NIMU, be.imu_count, be.prevTime, curTime, be.imu_head, head, k);
        sh_i[6] = head; sh_i[7] = k;
    }
    if (imu_here && t == 0) {
        const int head = sh_i[6], k = sh_i[7];
        sh_i[0] = head;          // first sample of the interval
        sh_i[1] = k - head + 1;  // number of samples incl. the first one with t >= curTime
        be.imu_head = k;         // that last sample is not popped
        be.n_imu_frame = sh_i[1];
        be.imu_frame_head = head;
        if (!be.initFirstPoseFlag) {  // initFirstIMUPose :1890-1909
            v3 aver = mk(0, 0, 0);
            for (int q = 0; q < sh_i[1]; q++) aver = add(aver, ld3(ia + (size_t)((head + q) % C.NIMU) * 3));
            aver = scl(1.0 / (double)sh_i[1], aver);
            m3 R0 = g2R(aver);
            double yaw = R2ypr(R0).x;
            R0 = mul(ypr2R(mk(-yaw, 0, 0)), R0);
            stm(be.Rs[0], R0);
            be.initFirstPoseFlag = 1;
        }
    }
    __syncthreads();
    if (imu_here) {
        int head = sh_i[0], n = sh_i[1];
        PreInt &P = c.pre[be.pre_idx[fc]];
        if (t == 0) {
            v3 a0 = ld3(ia + (size_t)(head % C.NIMU) * 3), g0 = ld3(ig + (size_t)(head % C.NIMU) * 3);
            if (!be.first_imu) { be.first_imu = 1; st3(be.acc_0, a0); st3(be.gyr_0, g0); }
            if (!P.valid) bf::preint_init(P, ld3(be.acc_0), ld3(be.gyr_0), ld3(be.Bas[fc]), ld3(be.Bgs[fc]));
        }
        __syncthreads();
        if (fc != 0) {
            // IntegrationBase::push_back + Estimator::processIMU for the n samples of the frame: the pipelined propagation on the ring's
            // interval, with the world-state recursion of Ps / Rs / Vs[fc] as its side job
            preint_load(P, pw);
            __shared__ double pi_fv[PREINT_MANY_LDS_DOUBLES];
            const PreintRing ring = {it, ia, ig, head, C.NIMU, be.prevTime, curTime, n};
            WorldStep ws = {ld3(be.acc_0), ld3(be.gyr_0), ld3(be.Ps[fc]), ld3(be.Vs[fc]), ldm(be.Rs[fc]), ld3(be.Bas[fc]), ld3(be.Bgs[fc]), ld3(be.g)};
            const int nb0 = P.n_buf;
            PH(111);
            preint_propagate_many<true>(P, pw, K, n, ring, ws, true, pi_fv);
            PH(112);
            if (t == 0 && nb0 + n > VIO_IMU_SLOT_CAP) be.overflow |= 2;
            if (t == 64) {
                stm(be.Rs[fc], ws.R); st3(be.Ps[fc], ws.P); st3(be.Vs[fc], ws.V);
                st3(be.acc_0, ws.a0); st3(be.gyr_0, ws.g0);
            }
            __syncthreads();
        } else if (t == 0) {   // frame 0: no pre-integration yet, acc_0 / gyr_0 follow the samples
            const int idx = (head + n - 1) % C.NIMU;
            st3(be.acc_0, ld3(ia + (size_t)idx * 3)); st3(be.gyr_0, ld3(ig + (size_t)idx * 3));
        }
        if (fc != 0) preint_store(P, pw);
        if (t == 0) be.prevTime = curTime;
        __syncthreads();
    }
    PH(109);
    if constexpr (EXCALIB) {
        // ---- InitialEXRotation::CalibrationExRotation (estimator.cpp:208-226): before triangulateWithDepth, which already uses a rotation
        // calibrated in this frame
        __shared__ ExShared exs;
        if (be.ex_pending && fc != 0)
            ex_calibrate(B, c, s, fc, nlm, (double *)(((uintptr_t)htab + 15) & ~(uintptr_t)15), scratch, sred, exs);
    }
    // ---- triangulateWithDepth (feature_manager.cpp:386-543); the dynamic initialisation triangulates after its SfM instead (estimator.cpp:921-933)
    if (!cfg.use_imu && be.solver_flag == 1) init_frame_pose_by_pnp(c, fc, c.res, sred);   // estimator.cpp:321-322 (VO mode, NON_LINEAR only)
    if (!(cfg.dynamic_init && be.solver_flag == 0)) triangulate_with_depth(c, nlm);
    __syncthreads();
    PH(110);
    if (t == 0) {
        be.processed = 1;
        be.frames_processed++;
        if (be.solver_flag == 0) {
            // static initialisation solves once the window is full; the dynamic one is decided by the host (vio_abi.hip run_dynamic_init)
            if (fc == W && !cfg.dynamic_init) { be.do_solve = 1; be.do_marg = 1; }
        } else { be.do_solve = 1; be.do_marg = 1; }
        // both initialisations are held while the sequence calibrates (estimator.cpp:236, :275); be_finish slides its window
        if constexpr (EXCALIB) { if (be.ex_pending) { be.do_solve = 0; be.do_marg = 0; } }
    }
}
template __global__ void be_ingest_kernel<false>(Batch, const uint16_t *, size_t, IngestSrc);
template __global__ void be_ingest_kernel<true>(Batch, const uint16_t *, size_t, IngestSrc);

// ====================================================================================================== dynamic init hand-over
// After a successful host-side initialStructure (dyninit_host.cpp) the host has written Ps / Rs / Vs / Bgs / Bas / g of sequence
// `seq`: re-propagate the window pre-integrations at the new gyroscope bias (estimator.cpp:829-836) and triangulate with the new
// poses (solveOdometry -> triangulateWithDepth, :921-933).  The regular be_solve / be_marg launches follow.
// `samples` = (dt, acc[3], gyr[3]) of every IMU step of window slot j in [offs[j], offs[j + 1]), rebuilt by the host from its mirror of
// all_image_frame: slots that absorbed dropped frames (MARGIN_SECOND_NEW while INITIAL, estimator.cpp:1651-1687) hold more steps than
// the per-slot sample buffer on the device keeps (the reference's buffers are unbounded vectors).
__global__ __launch_bounds__(256) void be_dyn_finalize_kernel(Batch B, int seq, const double *samples, const int *offs) {
    __shared__ PreWork pw;
    Ctx c = make_ctx(B, seq);
    BeSeq &be = *c.be;
    const vio_config &cfg = c.C->c;
    const int t = threadIdx.x, nt = blockDim.x, W = c.W;
    for (int j = 0; j <= W; j++) {
        PreInt &p = c.pre[be.pre_idx[j]];
        if (!p.valid) continue;
        if (t == 0) {
            v3 la = ld3(p.lin_acc), lg = ld3(p.lin_gyr);
            p.sum_dt = 0;
            st3(p.acc0, la); st3(p.gyr0, lg);
            p.dp[0] = p.dp[1] = p.dp[2] = 0; p.dv[0] = p.dv[1] = p.dv[2] = 0;
            p.dq[0] = 1; p.dq[1] = p.dq[2] = p.dq[3] = 0;
            p.lin_ba[0] = p.lin_ba[1] = p.lin_ba[2] = 0;
            st3(p.lin_bg, ld3(be.Bgs[j]));
        }
        for (int i = t; i < 225; i += nt) { pw.J[i] = ((i / 15) == (i % 15)) ? 1.0 : 0.0; pw.Pm[i] = 0; }
        __syncthreads();
        for (int q = offs[j]; q < offs[j + 1]; q++) {
            const double *sm = samples + (size_t)q * 7;
            preint_propagate(p, pw, *c.K, sm[0], ld3(sm + 1), ld3(sm + 4));
        }
        preint_store(p, pw);
    }
    __syncthreads();
    triangulate_with_depth(c, be.n_lm);
}

// stage test of the device solvePnP: par6 = (rvec, tvec) in / out; trace4 (may be null) = outer iterations, lambda escalations, final
// lambda_lg10, all six parameters finite
__global__ __launch_bounds__(256) void be_stage_pnp_kernel(const double *pts, int n, double *par6, int *trace4) {
    __shared__ double sh_par[6], sh_prev[6], sw[256];
    if (threadIdx.x < 6) sh_par[threadIdx.x] = par6[threadIdx.x];
    __syncthreads();
    pnp_refine_block(pts, n, sh_par, sh_prev, sw, trace4);
    if (threadIdx.x < 6) par6[threadIdx.x] = sh_par[threadIdx.x];
    if (trace4 && threadIdx.x == 0) {
        bool fin = true;
        for (int i = 0; i < 6; i++) fin = fin && isfinite(sh_par[i]);
        trace4[3] = fin ? 1 : 0;
    }
}
// cv::Rodrigues as the solve uses it, one thread per item (vio_stage_rodrigues): mode 0 r[3] -> R[9], dR/dr[27]; mode 1 R[9] -> r[3]
__global__ void be_stage_rodrigues_kernel(int mode, int n, const double *in, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) {
        const v3 r = ld3(in + 3 * (size_t)i);
        const m3 Rm = pnp_rodrigues(r);
        m3 dR[3];
        pnp_rodrigues_jac(r, Rm, dR);
        double *o = out + 36 * (size_t)i;
        stm(o, Rm);
        for (int k = 0; k < 3; k++) stm(o + 9 + 9 * k, dR[k]);
    } else
        st3(out + 3 * (size_t)i, pnp_rodrigues_inv(ldm(in + 9 * (size_t)i)));
}

// InitialEXRotation::solveRelativeR on one set of correspondences (vio_stage_relative_r): corres6[n][6] = (x, y, z) in frame l, (x, y, z) in
// frame r; grid 1, 256 threads, dynamic LDS 40 n + 64 bytes.  The same device code as the calibration phase of be_ingest<true>.
__global__ __launch_bounds__(256) void be_stage_relative_r_kernel(int n, const double *corres6, double *R9, int *detail8) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_rr[];
    __shared__ ExShared S;
    double *X1 = (double *)smem_rr, *Y1 = X1 + n, *X2 = Y1 + n, *Y2 = X2 + n;
    int *st = (int *)(Y2 + n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {   // cv::Point2f(corres[i].first(0), corres[i].first(1)) ...
        X1[i] = (double)(float)corres6[6 * i]; Y1[i] = (double)(float)corres6[6 * i + 1];
        X2[i] = (double)(float)corres6[6 * i + 3]; Y2[i] = (double)(float)corres6[6 * i + 4];
    }
    __syncthreads();
    ex_relative_r(n, X1, Y1, X2, Y2, st, S);
    if (threadIdx.x < 9) R9[threadIdx.x] = S.Rout[threadIdx.x];
    if (detail8 && threadIdx.x == 0) {   // (S.R.maxGood and the votes are defined only when the RANSAC ran / a model was found)
        const bool ran = n >= 9, ok = ran && S.ok;
        detail8[0] = ok ? 1 : 0;
        detail8[1] = ran ? S.R.maxGood : 0;
        for (int k = 0; k < 4; k++) detail8[2 + k] = ok ? S.cnt[k] : 0;
        detail8[6] = ok ? S.win : 0;
        detail8[7] = ok ? S.flip : 0;
    }
}

// IntegrationBase::push_back x n followed by IMUFactor::Evaluate, through the same device code the pipeline uses.
__global__ __launch_bounds__(256) void be_stage_imu_kernel(vio_config cfg, PreInt *P, int n, const double *dt, const double *acc,
                                                            const double *gyr, const double *par /*pi7 sbi9 pj7 sbj9*/, double g_norm,
                                                            double *preint_out, double *r15, double *J480) {
    __shared__ PreWork pw;
    const int t = threadIdx.x;
    preint_load(*P, pw);
    for (int q = 0; q < n; q++) preint_propagate(*P, pw, cfg, dt[q], ld3(acc + 3 * q), ld3(gyr + 3 * q));
    preint_store(*P, pw);
    if (t == 0) {
        PreInt &p = *P;
        preint_out[0] = p.dp[0]; preint_out[1] = p.dp[1]; preint_out[2] = p.dp[2];
        for (int k = 0; k < 4; k++) preint_out[3 + k] = p.dq[k];
        preint_out[7] = p.dv[0]; preint_out[8] = p.dv[1]; preint_out[9] = p.dv[2];
        preint_out[10] = p.sum_dt;
        for (int k = 0; k < 225; k++) { preint_out[11 + k] = p.jac[k]; preint_out[236 + k] = p.cov[k]; }
        double raw[15], Jr[450];
        v3 G = mk(0, 0, g_norm);
        bf::imu_raw_residual(p, G, par, par + 7, par + 16, par + 23, raw);
        bf::imu_raw_jacobian(p, G, par, par + 7, par + 16, par + 23, Jr);
        for (int r = 0; r < 15; r++) {
            double sacc = 0;
            for (int k = 0; k <= r; k++) sacc += p.sqrt_info[r * 15 + k] * raw[k];
            r15[r] = sacc;
        }
        // whitened Jacobians in the reference's global layout: 15x7, 15x9, 15x7, 15x9 (7th pose column = 0)
        for (int r = 0; r < 15; r++)
            for (int col = 0; col < 30; col++) {
                double sacc = 0;
                for (int k = 0; k <= r; k++) sacc += p.sqrt_info[r * 15 + k] * Jr[k * 30 + col];
                if (col < 6) J480[r * 7 + col] = sacc;
                else if (col < 15) J480[105 + r * 9 + (col - 6)] = sacc;
                else if (col < 21) J480[240 + r * 7 + (col - 15)] = sacc;
                else J480[345 + r * 9 + (col - 21)] = sacc;
            }
        for (int r = 0; r < 15; r++) { J480[r * 7 + 6] = 0; J480[240 + r * 7 + 6] = 0; }
    }
}

// out686 of the pre-integration harnesses = delta_p(3) delta_q(wxyz) delta_v(3) sum_dt jacobian(225) covariance(225) sqrt_info(225)
__device__ __forceinline__ void stage_preint_out(const PreInt &p, double *out686) {
    if (threadIdx.x == 0) {
        out686[0] = p.dp[0]; out686[1] = p.dp[1]; out686[2] = p.dp[2];
        for (int k = 0; k < 4; k++) out686[3 + k] = p.dq[k];
        out686[7] = p.dv[0]; out686[8] = p.dv[1]; out686[9] = p.dv[2];
        out686[10] = p.sum_dt;
    }
    for (int k = threadIdx.x; k < 225; k += blockDim.x) { out686[11 + k] = p.jac[k]; out686[236 + k] = p.cov[k]; out686[461 + k] = p.sqrt_info[k]; }
}
// The two propagation routines of the pipeline on one sample list, for comparison with each other and with the definition: mode 0 = n calls
// of preint_propagate (be_dyn_finalize, be_marg's repropagation), 1 = preint_propagate_many(append = false), 2 = the same with append = true
// (the MARGIN_SECOND_NEW merge: the samples are also filed into P's buffers, n_buf saturating at VIO_IMU_SLOT_CAP).  preint_store refreshes
// sqrt_info as everywhere.
__global__ __launch_bounds__(256) void be_stage_preint_kernel(vio_config cfg, PreInt *P, int n, const double *dt, const double *acc,
                                                               const double *gyr, int mode, double *out686) {
    __shared__ PreWork pw;
    __shared__ double lds_fv[PREINT_MANY_LDS_DOUBLES];
    preint_load(*P, pw);
    if (mode == 0)
        for (int q = 0; q < n; q++) preint_propagate(*P, pw, cfg, dt[q], ld3(acc + 3 * q), ld3(gyr + 3 * q));
    else {
        PreintNoSide none;
        preint_propagate_many<false>(*P, pw, cfg, n, PreintArrays{dt, (const double (*)[3])acc, (const double (*)[3])gyr}, none, mode == 2, lds_fv);
    }
    preint_store(*P, pw);
    stage_preint_out(*P, out686);
}
// What be_ingest adds to preint_propagate_many: the n samples of a ring's interval as the source (PreintRing) and the world-state step
// (WorldStep) as the side job, append on.  world31 (in and out) = WorldStep's fields acc_0 gyr_0 P V R(9) Ba Bg g, then the overflow
// bits by be_ingest's rule.
__global__ __launch_bounds__(256) void be_stage_preint_ring_kernel(vio_config cfg, PreInt *P, PreintRing ring, double *world31, double *out686) {
    __shared__ PreWork pw;
    __shared__ double lds_fv[PREINT_MANY_LDS_DOUBLES];
    const double *w = world31;
    const int t = threadIdx.x;
    preint_load(*P, pw);
    WorldStep ws = {ld3(w), ld3(w + 3), ld3(w + 6), ld3(w + 9), ldm(w + 12), ld3(w + 21), ld3(w + 24), ld3(w + 27)};
    const int nb0 = P->n_buf;
    preint_propagate_many<true>(*P, pw, cfg, ring.n, ring, ws, true, lds_fv);
    if (t == 0) world31[30] = nb0 + ring.n > VIO_IMU_SLOT_CAP ? 2 : 0;
    if (t == 64) { st3(world31, ws.a0); st3(world31 + 3, ws.g0); st3(world31 + 6, ws.P); st3(world31 + 9, ws.V); stm(world31 + 12, ws.R); }
    preint_store(*P, pw);
    stage_preint_out(*P, out686);
}
