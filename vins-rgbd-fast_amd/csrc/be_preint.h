// IMU pre-integration, block-cooperative (IntegrationBase::propagate / push_back): shared by be_ingest.hip (the frame's IMU, the hand-over
// of the dynamic initialisation), be_solve_common.h (repropagate_window), be_kernels.hip (the window slide) and the preint stage kernels.
#pragma once
#include "be_ctx.h"
#include "be_linalg.h"

namespace {

// ------------------------------------------------------------------ IntegrationBase::propagate, block-cooperative
// LDS workspace: sJ sP sFJ sFP (225 each) sF (225) sV (270)
struct PreWork { double J[225], Pm[225], FJ[225], FP[225], F[225], V[270]; };
// PI_CH (kernels.h): samples per chunk of the pipelined propagation (F / V of a chunk live in LDS: 8 x 495 doubles)
__device__ __forceinline__ void preint_load(const PreInt &p, PreWork &w) {
    for (int i = threadIdx.x; i < 225; i += blockDim.x) { w.J[i] = p.jac[i]; w.Pm[i] = p.cov[i]; }
    __syncthreads();
}
// Also refreshes the whitening matrix of the IMU factor: M = chol(cov)^-1 (lower triangular), M^T M = cov^-1.
// The reference uses LLT(cov^-1).L^T (imu_factor.h:66-69); both satisfy M^T M = cov^-1, so J^T J, J^T r and |r|^2 - the only
// quantities the solver and the marginalisation consume - are identical up to round-off (DESIGN.md "equivalent whitening").
__device__ __forceinline__ void preint_store(PreInt &p, PreWork &w) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int i = t; i < 225; i += blockDim.x) { p.jac[i] = w.J[i]; p.cov[i] = w.Pm[i]; }
    if (t < 225) { int i = t / 15, j = t - i * 15; w.FJ[t] = 0.5 * (w.Pm[i * 15 + j] + w.Pm[j * 15 + i]); }
    __syncthreads();
    for (int j = 0; j < 15; j++) {
        if (t == 0) { double d = w.FJ[j * 15 + j]; w.FJ[j * 15 + j] = (d > 0.0 && isfinite(d)) ? sqrt(d) : 0.0; }
        __syncthreads();
        double l = w.FJ[j * 15 + j];
        if (t > j && t < 15) w.FJ[t * 15 + j] = l > 0.0 ? w.FJ[t * 15 + j] / l : 0.0;
        __syncthreads();
        if (t < 225) { int i = t / 15, k = t - i * 15; if (k > j && i >= k) w.FJ[t] -= w.FJ[i * 15 + j] * w.FJ[k * 15 + j]; }
        __syncthreads();
    }
    if (t < 225) w.FP[t] = 0;
    __syncthreads();
    if (t < 15) {
        double x[15];
        bool ok = true;
        for (int i = 0; i < 15; i++) ok = ok && w.FJ[i * 15 + i] > 0.0;
        for (int i = 0; i < 15; i++) {
            double sacc = (i == t) ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) sacc -= w.FJ[i * 15 + k] * x[k];
            x[i] = ok ? sacc / w.FJ[i * 15 + i] : 0.0;
            w.FP[i * 15 + t] = x[i];
        }
    }
    __syncthreads();
    if (t < 225) p.sqrt_info[t] = w.FP[t];
    __syncthreads();
}
// one step of the jacobian / covariance recursion on the LDS-resident matrices, all threads: J <- F J, P <- F P F^T + V Q V^T
// (integration_base.h:131-132).  N: the noise densities (acc_n, gyr_n, acc_w, gyr_w): the sequence's vio_calibration, or the vio_config
// of a stage harness
template <class N> __device__ __forceinline__ void preint_cov_step(PreWork &w, const double *Fk, const double *Vk, const N &c) {
    const int t = threadIdx.x;
    if (t < 225) {
        int i = t / 15, j = t - i * 15;
        double s1 = 0, s2 = 0;
        for (int u = 0; u < 15; u++) { s1 += Fk[i * 15 + u] * w.J[u * 15 + j]; s2 += Fk[i * 15 + u] * w.Pm[u * 15 + j]; }
        w.FJ[t] = s1; w.FP[t] = s2;
    }
    __syncthreads();
    if (t < 225) {
        int i = t / 15, j = t - i * 15;
        double s1 = 0;
        for (int u = 0; u < 15; u++) s1 += w.FP[i * 15 + u] * Fk[j * 15 + u];
        const double nn[6] = {c.acc_n * c.acc_n, c.gyr_n * c.gyr_n, c.acc_n * c.acc_n, c.gyr_n * c.gyr_n, c.acc_w * c.acc_w, c.gyr_w * c.gyr_w};
        double tt = 0;
        for (int u = 0; u < 18; u++) tt += Vk[i * 18 + u] * nn[u / 3] * Vk[j * 18 + u];
        w.J[t] = w.FJ[t];
        w.Pm[t] = s1 + tt;
    }
    __syncthreads();
}
// one propagate(dt, acc, gyr) on the LDS-resident jacobian/covariance; p's small state is updated by thread 0
template <class N> __device__ void preint_propagate(PreInt &p, PreWork &w, const N &c, double dt, v3 acc1, v3 gyr1) {
    if (threadIdx.x == 0) {
        bf::PreintStep o = bf::preint_midpoint(p, dt, acc1, gyr1, w.F, w.V);
        st3(p.dp, o.dp); st3(p.dv, o.dv);
        quat q = qnormalized(o.dq);
        p.dq[0] = q.w; p.dq[1] = q.x; p.dq[2] = q.y; p.dq[3] = q.z;
        p.sum_dt += dt;
        st3(p.acc0, acc1); st3(p.gyr0, gyr1);
    }
    __syncthreads();
    preint_cov_step(w, w.F, w.V, c);
}

// Sample sources of preint_propagate_many: get(q) yields dt, acc and gyr of sample q of the n to integrate.
struct PreintArrays {   // the samples as arrays (a slot's own buffers, a stage harness)
    const double *dt; const double (*acc)[3]; const double (*gyr)[3];
    __device__ __forceinline__ void get(int q, double &dt_q, double *acc_q, double *gyr_q) const {
        dt_q = dt[q];
        for (int k = 0; k < 3; k++) { acc_q[k] = acc[q][k]; gyr_q[k] = gyr[q][k]; }
    }
};
// Side jobs of preint_propagate_many: run by thread 64 (another wavefront than thread 0's) on the m staged samples of a chunk.
struct PreintNoSide { __device__ __forceinline__ void operator()(int, const double *, const double (*)[3], const double (*)[3]) {} };
// Estimator::processIMU's world-state recursion of a frame (estimator.cpp:142-152); acc_0 / gyr_0 are the estimator's, not the slot's
struct WorldStep {
    v3 a0, g0, P, V; m3 R; v3 Ba, Bg, g;
    __device__ __forceinline__ void operator()(int m, const double *dt_s, const double (*acc_s)[3], const double (*gyr_s)[3]) {
        for (int k = 0; k < m; k++) {
            const v3 acc = ld3(acc_s[k]), gyr = ld3(gyr_s[k]);
            const double dt = dt_s[k];
            v3 un_acc_0 = sub(mul(R, sub(a0, Ba)), g);
            v3 un_gyr = sub(scl(0.5, add(g0, gyr)), Bg);
            R = mul(R, q2R(deltaQ(scl(dt, un_gyr))));
            v3 un_acc_1 = sub(mul(R, sub(acc, Ba)), g);
            v3 un_acc = scl(0.5, add(un_acc_0, un_acc_1));
            P = add(add(P, scl(dt, V)), scl(dt * dt, scl(0.5, un_acc)));
            V = add(V, scl(dt, un_acc));
            a0 = acc; g0 = gyr;
        }
    }
};

// n propagate steps on the LDS-resident jacobian / covariance (preint_load'ed into w), IntegrationBase::push_back pipelined in chunks of
// PI_CH samples:
//   A  thread 0 runs the short delta-state recursion of the chunk and keeps the state before every step, thread 64 - another
//      wavefront - the caller's side job, and with IDLE_CLEARS the threads from 128 on clear the chunk's F / V (the caller then
//      launches more than 128 threads);
//   B  one lane per sample builds that step's F (15 x 15) and V (15 x 18) from the state before it, clearing them first without
//      IDLE_CLEARS (495 stores of one lane);
//   C  the jacobian / covariance recursion consumes them step by step.
// The arithmetic of n calls of preint_propagate (be_factors.h preint_state_step / preint_step_FV are the two halves of preint_midpoint)
// with the serial part of a step shrunk from the whole midpoint step to the recursion.  append: the samples are also filed into p's
// own buffers (IntegrationBase::push_back); the caller decides what running over VIO_IMU_SLOT_CAP means.  The per-frame integration of
// be_ingest and the merge of MARGIN_SECOND_NEW (estimator.cpp:1651-1687) both run this.
// lds_fv: PREINT_MANY_LDS_DOUBLES (kernels.h) doubles for F and V of a chunk, lent by the caller.
template <bool IDLE_CLEARS, class N, class Src, class Side>
__device__ void preint_propagate_many(PreInt &p, PreWork &w, const N &cfg, int n, const Src &src, Side &side, bool append, double *lds_fv) {
    const int t = threadIdx.x, nt = blockDim.x;
    double (*pm_F)[225] = (double (*)[225])lds_fv;
    double (*pm_V)[270] = (double (*)[270])(lds_fv + PI_CH * 225);
    __shared__ double pm_dt[PI_CH], pm_acc[PI_CH][3], pm_gyr[PI_CH][3];
    __shared__ bf::PreintPre pm_pre[PI_CH];
    const int nb0 = p.n_buf;
    const v3 lba = ld3(p.lin_ba), lbg = ld3(p.lin_bg);
    quat s_dq = mkq(p.dq[0], p.dq[1], p.dq[2], p.dq[3]);
    v3 s_dp = ld3(p.dp), s_dv = ld3(p.dv), s_a0 = ld3(p.acc0), s_g0 = ld3(p.gyr0);
    double s_sum = p.sum_dt;
    __syncthreads();
    for (int q0 = 0; q0 < n; q0 += PI_CH) {
        const int m = min(PI_CH, n - q0);
        if (t < m) {   // stage the chunk's samples
            const int q = q0 + t, nb = nb0 + q;
            double dt, acc[3], gyr[3];
            src.get(q, dt, acc, gyr);
            pm_dt[t] = dt;
            for (int k = 0; k < 3; k++) { pm_acc[t][k] = acc[k]; pm_gyr[t][k] = gyr[k]; }
            if (append && nb < VIO_IMU_SLOT_CAP) { p.dt_buf[nb] = dt; for (int k = 0; k < 3; k++) { p.acc_buf[nb][k] = acc[k]; p.gyr_buf[nb][k] = gyr[k]; } }
        }
        __syncthreads();
        if (t == 0) {
            for (int k = 0; k < m; k++) {
                const v3 acc = ld3(pm_acc[k]), gyr = ld3(pm_gyr[k]);
                pm_pre[k].dq = s_dq; pm_pre[k].acc0 = s_a0; pm_pre[k].gyr0 = s_g0;
                bf::preint_state_step(s_dq, s_dp, s_dv, s_a0, s_g0, lba, lbg, pm_dt[k], acc, gyr);
                s_sum += pm_dt[k];
                s_a0 = acc; s_g0 = gyr;
            }
        } else if (t == 64) {
            side(m, pm_dt, pm_acc, pm_gyr);
        } else if (IDLE_CLEARS && t >= 128) {   // (idle otherwise during the recursions)
            for (int q = t - 128; q < m * 225; q += nt - 128) (&pm_F[0][0])[q] = 0;
            for (int q = t - 128; q < m * 270; q += nt - 128) (&pm_V[0][0])[q] = 0;
        }
        __syncthreads();
        if (t < m) bf::preint_step_FV(pm_pre[t], lba, lbg, pm_dt[t], ld3(pm_acc[t]), ld3(pm_gyr[t]), pm_F[t], pm_V[t], !IDLE_CLEARS);
        __syncthreads();
        for (int k = 0; k < m; k++) preint_cov_step(w, pm_F[k], pm_V[k], cfg);
    }
    if (t == 0) {
        st3(p.dp, s_dp); st3(p.dv, s_dv);
        p.dq[0] = s_dq.w; p.dq[1] = s_dq.x; p.dq[2] = s_dq.y; p.dq[3] = s_dq.z;
        p.sum_dt = s_sum;
        st3(p.acc0, s_a0); st3(p.gyr0, s_g0);
        if (append) p.n_buf = min(nb0 + n, VIO_IMU_SLOT_CAP);
    }
    __syncthreads();
}

}  // namespace
