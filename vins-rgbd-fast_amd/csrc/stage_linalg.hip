// Stage entry points of the dense FP64 linear algebra (be_linalg.h) on its own: the LDS-tile Cholesky + triangular solves of ps_serial
// (be_phased.h) on a caller-supplied matrix, with the in-kernel time of each part -- the parity anchor (numpy) and the tuning harness of
// that code.  Replaces nothing of the reference by itself: the reference reaches this arithmetic through Ceres' DENSE_SCHUR
// (estimator.cpp:1251-1263, Eigen LLT underneath).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stage_util.h"
#include "be_linalg.h"

namespace {

__global__ __launch_bounds__(512) void be_stage_chol_kernel(int nb, int reps, int blocks_mode, const double *S, const double *rhs, double *Lout, double *xout,
                                                             float *ticks /*[3]: factor, backward, wall ticks per microsecond*/) {
    extern __shared__ __attribute__((aligned(16))) double T[];
    const int t = threadIdx.x, nt = blockDim.x, n = 16 * nb, ntile = nb * (nb + 1) / 2;
    double *xs = T + (size_t)ntile * 256, *dinv = xs + n;
    __shared__ int flag;
    __shared__ float tm[4];
    if (t < 4) tm[t] = 0;
    long long tf = 0, tb = 0;
    bool ok = true;
    if (blocks_mode > 0) {
        // micro modes (tuning): 1 = chol_diag_tile alone on wavefront 0, 2 = the same with wavefront 4 (its SIMD mate) running trailing
        // updates beside it, 3 = one chol_panel_tile per wavefront, 4 = 8 tile updates per wavefront
        const int wave = t >> 6, lane = t & 63, li = lane & 15, lk = lane >> 4;
        for (int q = t; q < ntile * 256; q += nt) {
            int ti, tj;
            tri_decode(q >> 8, ti, tj);
            T[tl_idx(ti, tj, (q >> 4) & 15, q & 15)] = S[(size_t)(16 * ti + ((q >> 4) & 15)) * n + 16 * tj + (q & 15)];
        }
        __syncthreads();
        long long acc_t = 0;
        for (int rep = 0; rep < reps; rep++) {
            if (wave == 0 && (blocks_mode == 1 || blocks_mode == 2))
                for (int q = lane; q < 256; q += 64) T[q] = S[(size_t)(q >> 4) * n + (q & 15)] + (q >> 4 == (q & 15) ? 1.0 : 0.0);
            __syncthreads();
            const long long t0 = (long long)wall_clock64();
            if (blocks_mode == 1) { if (wave == 0) { const long long c0 = (long long)clock64(); chol_diag_tile(T, dinv, &flag); if (lane == 0) ticks[1] = (float)((long long)clock64() - c0); } }
            else if (blocks_mode == 2) {
                if (wave == 0) chol_diag_tile(T, dinv, &flag);
                else if (wave == 4 && nb >= 3)
                    for (int it = 0; it < 6; it++) {
                        v4f64 a;
                        for (int r = 0; r < 4; r++) a[r] = T[tl_idx(2, 1, lk + 4 * r, li)];
                        for (int kk = 0; kk < 4; kk++) a = __builtin_amdgcn_mfma_f64_16x16x4f64(-T[tl_idx(2, 0, li, 4 * kk + lk)], T[tl_idx(1, 0, li, 4 * kk + lk)], a, 0, 0, 0);
                        for (int r = 0; r < 4; r++) T[tl_idx(2, 1, lk + 4 * r, li)] = a[r];
                    }
            } else if (blocks_mode == 4) {
                // 256 dependent FP64 fused multiply-adds, then 64 dependent v_rsq_f64, on wavefront 0; clock64 ticks into ticks[1..2]
                if (wave == 0) {
                    double v = T[lane];
                    const long long c0 = (long long)clock64();
#pragma unroll
                    for (int k = 0; k < 256; k++) v = __builtin_fma(v, 1.0000001, 1e-9);
                    const long long c1 = (long long)clock64();
#pragma unroll
                    for (int k = 0; k < 64; k++) v = __builtin_amdgcn_rsq(v + 2.0);
                    const long long c2 = (long long)clock64();
                    T[lane] = v;
                    if (lane == 0) { ticks[1] = (float)(c1 - c0); ticks[2] = (float)(c2 - c1); }
                }
            } else if (blocks_mode == 6) {
                // FP64 matrix-core timing on wavefront 0 (clock64 ticks): [1] 64 MFMAs chained on one accumulator, [2] 64 alternating
                // between two accumulators, [3] 32 x (MFMA -> v_mul on its result -> MFMA), [4] 64 dependent v_rsq_f64
                if (wave == 0) {
                    v4f64 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
                    double x = T[lane], y = T[64 + lane];
                    const long long c0 = (long long)clock64();
#pragma unroll
                    for (int k = 0; k < 64; k++) a = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    double s0 = a[0] + a[1] + a[2] + a[3];
                    const long long c1 = (long long)clock64();
#pragma unroll
                    for (int k = 0; k < 32; k++) { a = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a, 0, 0, 0); b = __builtin_amdgcn_mfma_f64_16x16x4f64(y, x, b, 0, 0, 0); }
                    __builtin_amdgcn_sched_barrier(0);
                    s0 += a[0] + b[0];
                    const long long c2 = (long long)clock64();
#pragma unroll
                    for (int k = 0; k < 32; k++) { a = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a, 0, 0, 0); x = a[0] * 1e-3; }
                    __builtin_amdgcn_sched_barrier(0);
                    s0 += a[0];
                    const long long c3 = (long long)clock64();
                    double z = s0 * 1e-300 + 2.0;
#pragma unroll
                    for (int k = 0; k < 64; k++) z = __builtin_amdgcn_rsq(z) + 1.5;
                    __builtin_amdgcn_sched_barrier(0);
                    const long long c4 = (long long)clock64();
                    T[lane] = s0 + z;
                    if (lane == 0) { ticks[1] = (float)(c1 - c0); ticks[2] = (float)(c2 - c1); ticks[3] = (float)(c3 - c2); ticks[4] = (float)(c4 - c3); }
                }
            } else if (blocks_mode == 3) { if (nb >= 4 && wave < 3) chol_panel_tile(T + ((size_t)((wave + 1) * (wave + 2) / 2) << 8), T, dinv); }
            __syncthreads();
            acc_t += (long long)wall_clock64() - t0;
        }
        if (t == 0 && blockIdx.x == 0) { ticks[0] = (float)acc_t / reps; if (blocks_mode != 4 && blocks_mode != 1 && blocks_mode != 6) { ticks[1] = ticks[2] = 0; } if (blocks_mode != 6) { ticks[3] = ticks[4] = 0; } }
        return;
    }
    for (int rep = 0; rep < reps; rep++) {
        for (int q = t; q < ntile * 256; q += nt) {
            int ti, tj;
            tri_decode(q >> 8, ti, tj);
            const int r = (q >> 4) & 15, c = q & 15;
            T[tl_idx(ti, tj, r, c)] = S[(size_t)(16 * ti + r) * n + 16 * tj + c];
        }
        for (int q = t; q < n; q += nt) xs[q] = rhs[q];
        __syncthreads();
        const long long t0 = (long long)wall_clock64();
        ok = chol_tiles(T, nb, &flag, dinv, tm, xs) && ok;
        __syncthreads();
        const long long t1 = (long long)wall_clock64();
        chol_backward_tiles_wave(T, nb, xs, dinv);
        __syncthreads();
        const long long t2 = (long long)wall_clock64();
        tf += t1 - t0; tb += t2 - t1;
    }
    if (blockIdx.x != 0) return;
    for (int q = t; q < ntile * 256; q += nt) {
        int ti, tj;
        tri_decode(q >> 8, ti, tj);
        const int r = (q >> 4) & 15, c = q & 15;
        if (ti == tj && c > r) continue;   // (the strict upper triangle of a diagonal tile holds L^-1 of the block)
        Lout[(size_t)(16 * ti + r) * n + 16 * tj + c] = T[tl_idx(ti, tj, r, c)];
    }
    for (int q = t; q < n; q += nt) xout[q] = ok ? xs[q] : nan("");
    if (t == 0) { ticks[0] = (float)tf / reps; ticks[1] = (float)tb / reps; for (int k = 0; k < 3; k++) ticks[2 + k] = tm[k] / reps; }
}

// the streaming factorisation of ps_serial_big (windows beyond 10 keyframes): tiles in HBM / L2, one block column at a time through LDS
__global__ __launch_bounds__(512) void be_stage_chol_stream_kernel(int nb, int reps, const double *S, const double *rhs, double *Tg, double *Lout, double *xout,
                                                                    float *ticks) {
    extern __shared__ __attribute__((aligned(16))) double colbuf[];
    const int t = threadIdx.x, nt = blockDim.x, n = 16 * nb, ntile = nb * (nb + 1) / 2;
    double *T = Tg + (size_t)blockIdx.x * ntile * 256;
    double *xs = colbuf + ((size_t)2 * nb + 1) * 256, *dinv = xs + n;   // two block columns + the look-ahead tile (chol_tiles_stream)
    __shared__ int flag;
    __shared__ float tm[4];
    if (t < 4) tm[t] = 0;
    long long tf = 0, tb = 0;
    bool ok = true;
    for (int rep = 0; rep < reps; rep++) {
        for (int q = t; q < ntile * 256; q += nt) {
            int ti, tj;
            tri_decode(q >> 8, ti, tj);
            T[tl_idx(ti, tj, (q >> 4) & 15, q & 15)] = S[(size_t)(16 * ti + ((q >> 4) & 15)) * n + 16 * tj + (q & 15)];
        }
        for (int q = t; q < n; q += nt) xs[q] = rhs[q];
        __threadfence_block();
        __syncthreads();
        const long long t0 = (long long)wall_clock64();
        ok = chol_tiles_stream(T, nb, colbuf, &flag, dinv, xs, tm) && ok;
        __syncthreads();
        const long long t1 = (long long)wall_clock64();
        if (ok) chol_backward_tiles_wave(T, nb, xs, dinv);
        __syncthreads();
        const long long t2 = (long long)wall_clock64();
        tf += t1 - t0; tb += t2 - t1;
    }
    if (blockIdx.x != 0) return;
    for (int q = t; q < ntile * 256; q += nt) {
        int ti, tj;
        tri_decode(q >> 8, ti, tj);
        const int r = (q >> 4) & 15, c = q & 15;
        if (ti == tj && c > r) continue;
        Lout[(size_t)(16 * ti + r) * n + 16 * tj + c] = T[tl_idx(ti, tj, r, c)];
    }
    for (int q = t; q < n; q += nt) xout[q] = ok ? xs[q] : nan("");
    __syncthreads();
    if (t == 0) { ticks[0] = (float)tf / reps; ticks[1] = (float)tb / reps; ticks[2] = tm[0] / reps; ticks[3] = tm[1] / reps; ticks[4] = tm[2] / reps; }
}

}  // namespace

// wall-clock ticks of a stage kernel in microseconds
static void stage_ticks_to_usec(const float *ticks, int count, double *usec) {
    int rate_khz = 100000, dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || rate_khz <= 0) rate_khz = 100000;
    if (usec) for (int k = 0; k < count; k++) usec[k] = ticks[k] / (rate_khz * 1e-3);
}

// the streaming path (ps_serial_big): tiles in HBM, one block column in LDS; blocks = -7 forces it for nb <= 11 (bit-for-bit against the LDS path)
static int stage_chol_stream(int nb, int reps, int blocks, const double *S, const double *rhs, double *L_out, double *x_out, double *usec2) {
    const size_t n = 16 * (size_t)nb, ntile = (size_t)nb * (nb + 1) / 2, lds = (((size_t)2 * nb + 1) * 256 + 2 * n) * sizeof(double);
    const int nblk = blocks < 0 ? 1 : blocks;
    DevBuf<double> dS, dr, dL, dx, dT;
    DevBuf<float> dt;
    float ht[5] = {0, 0, 0, 0, 0};
    HIPCHK(hipFuncSetAttribute((const void *)be_stage_chol_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(dS.alloc(n * n)); HIPCHK(dr.alloc(n)); HIPCHK(dL.alloc(n * n));
    HIPCHK(dx.alloc(n)); HIPCHK(dt.alloc(8)); HIPCHK(dT.alloc((size_t)nblk * ntile * 256));
    HIPCHK(dS.upload(S, n * n)); HIPCHK(dr.upload(rhs, n));
    HIPCHK(dL.upload(L_out, n * n));
    be_stage_chol_stream_kernel<<<nblk, 512, lds>>>(nb, reps, dS, dr, dT, dL, dx, dt);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dL.download(L_out, n * n)); HIPCHK(dx.download(x_out, n));
    HIPCHK(dt.download(ht, 5));
    stage_ticks_to_usec(ht, 5, usec2);
    return VIO_OK;
}

// Harness of sym_eig_hbm (be_linalg.h): one workgroup decomposes the symmetric n x n matrix A (row-major, n <= 512) in place in HBM.  evals[n] (unsorted),
// evecs[n * n] (evecs[i * n + k] = component i of the eigenvector of evals[k]), usec = the decomposition's time on the device.
namespace {
__global__ __launch_bounds__(512) void be_stage_sym_eig_kernel(double *A, int n, double *evals, float *ticks) {
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) double eig_wk[];
    const long long t0 = (long long)wall_clock64();
    sym_eig_hbm(A, n, n, eig_wk, sred, ticks);
    for (int j = threadIdx.x; j < n; j += blockDim.x) evals[j] = eig_wk[j];
    __syncthreads();
    if (threadIdx.x == 0) ticks[0] = (float)((long long)wall_clock64() - t0);
}
}  // namespace
extern "C" int vio_stage_sym_eig(int n, const double *A, double *evals, double *evecs, double *usec) {   // usec[4]: total, tridiagonalisation, accumulation, QL
    if (n < 2 || n > SYM_EIG_HBM_MAX || !A || !evals || !evecs) return VIO_EINVAL;
    const size_t lds = (size_t)SYM_EIG_HBM_LDS_DOUBLES * sizeof(double);
    DevBuf<double> dA, dv;
    DevBuf<float> dt;
    float ht[4] = {0, 0, 0, 0};
    HIPCHK(dA.alloc((size_t)n * n)); HIPCHK(dv.alloc((size_t)n)); HIPCHK(dt.alloc(4));
    HIPCHK(dA.upload(A, (size_t)n * n));
    be_stage_sym_eig_kernel<<<1, 512, lds>>>(dA, n, dv, dt);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dA.download(evecs, (size_t)n * n)); HIPCHK(dv.download(evals, (size_t)n));
    HIPCHK(dt.download(ht, 4));
    stage_ticks_to_usec(ht, 4, usec);
    return VIO_OK;
}

static int stage_chol_blocked(int nb, int nt, const double *S, const double *rhs, double *L_out, double *x_out);

// S: [16 nb][16 nb] row-major symmetric positive definite, rhs: [16 nb].  L_out (row-major, lower triangle written, the rest left as
// passed in), x_out = S^-1 rhs, usec5 = {factorisation + forward substitution, backward substitution, and of the factorisation as
// thread 0 sees it: panel phases, diagonal block + trailing update, barrier wait} in microseconds of one workgroup (mean over reps;
// `blocks` identical workgroups run side by side).
extern "C" int vio_stage_chol(int nb, int reps, int blocks, const double *S, const double *rhs, double *L_out, double *x_out, double *usec5) {
    double *usec2 = usec5;
    if (nb < 1 || nb > 24 || reps < 1 || blocks == 0 || blocks < -9 || !S || !rhs || !L_out || !x_out) return VIO_EINVAL;
    if (blocks <= -8) return nb <= 21 ? stage_chol_blocked(nb, blocks == -8 ? 1024 : 512, S, rhs, L_out, x_out) : VIO_EINVAL;
    if (nb > 11 && blocks < 0 && blocks != -7) return VIO_EINVAL;
    if (nb > 11 || blocks == -7) return stage_chol_stream(nb, reps, blocks, S, rhs, L_out, x_out, usec5);
    const size_t n = 16 * (size_t)nb, ntile = (size_t)nb * (nb + 1) / 2, lds = (ntile * 256 + 2 * n) * sizeof(double);
    DevBuf<double> dS, dr, dL, dx;
    DevBuf<float> dt;
    float ht[5] = {0, 0, 0, 0, 0};
    HIPCHK(hipFuncSetAttribute((const void *)be_stage_chol_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(dS.alloc(n * n)); HIPCHK(dr.alloc(n)); HIPCHK(dL.alloc(n * n));
    HIPCHK(dx.alloc(n)); HIPCHK(dt.alloc(8));
    HIPCHK(dS.upload(S, n * n)); HIPCHK(dr.upload(rhs, n));
    HIPCHK(dL.upload(L_out, n * n));
    be_stage_chol_kernel<<<blocks < 0 ? 1 : blocks, 512, lds>>>(nb, reps, blocks < 0 ? -blocks : 0, dS, dr, dL, dx, dt);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dL.download(L_out, n * n)); HIPCHK(dx.download(x_out, n));
    HIPCHK(dt.download(ht, 5));
    stage_ticks_to_usec(ht, 5, usec2);
    return VIO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ABI 9: the remaining primitives
// One workgroup each, the be_linalg.h routine called directly (no restatement), at the block size of its production call site unless the entry takes
// one.  Eigenvector arrays out: evecs[i * n + k] = component i of the eigenvector of evals[k] (the convention of vio_stage_sym_eig).
#define JAC_LDS_MAX 96    // jacobi_block with A and V in LDS (2 n^2 doubles); beyond, in HBM as marg_exact runs it
#define JAC_HBM_MAX 256   // cs / sn / pp / qq below hold n / 2 + 1 entries
namespace {
__global__ __launch_bounds__(1024) void be_stage_jacobi_kernel(int mode, int n, double *Ag, double *Vg, int *sweeps) {
    extern __shared__ __attribute__((aligned(16))) double jl[];
    __shared__ double cs[JAC_HBM_MAX / 2 + 1], sn[JAC_HBM_MAX / 2 + 1], sred[64];
    __shared__ int pp[JAC_HBM_MAX / 2 + 1], qq[JAC_HBM_MAX / 2 + 1], sw;
    const int t = threadIdx.x, nt = blockDim.x;
    const bool hbm = mode == 3 || (mode == 1 && n > JAC_LDS_MAX);
    double *A = hbm ? Ag : jl, *V = hbm ? Vg : jl + (size_t)n * n;
    if (!hbm) for (int w = t; w < n * n; w += nt) A[w] = Ag[w];
    if (t == 0) sw = 0;
    __syncthreads();
    if (mode == 0) { if (t == 0) jacobi_small(A, V, n); }
    else if (mode == 2) { if (t < 64) { const int s = jacobi_wave16(A, V, n, n, cs, sn, pp, qq); if (t == 0) sw = s; } }
    else { const int s = jacobi_block(A, V, n, n, cs, sn, pp, qq, sred); if (t == 0) sw = s; }
    __syncthreads();
    if (!hbm) for (int w = t; w < n * n; w += nt) { Ag[w] = A[w]; Vg[w] = V[w]; }
    if (t == 0) *sweeps = sw;
}

// sym_eig_tridiag / sym_eig_tridiag_mt + tridiag_ql_wave with be_prior_factor_kernel's layout: LDS with leading dimension n | 1, or HBM with n, and
// one call site per address space
__global__ __launch_bounds__(512) void be_stage_sym_eig_lds_kernel(int n, int one_wave, int in_hbm, const double *A, double *Ag, double *evals, double *evecs) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) double se_lds[];
    const bool in_lds = !in_hbm;
    const int ldj = in_lds ? (n | 1) : n;
    double *As = in_lds ? se_lds : Ag;
    for (int w = t; w < n * n; w += nt) { int i = w / n, j = w - i * n; As[i * ldj + j] = A[w]; }
    __syncthreads();
    __shared__ double ev_d[6 * VIO_MAXW + 16], ev_e[6 * VIO_MAXW + 16], ev_g[6 * VIO_MAXW + 16];
    __shared__ double ev_part[8 * EIG_LD];
    if (in_lds) {
        double *Al = se_lds;
        if (!one_wave) sym_eig_tridiag_mt(Al, n, ldj, ev_d, ev_e, ev_g, ev_part);
        else sym_eig_tridiag(Al, n, ldj, ev_d, ev_e, ev_g, sred);
        tridiag_ql_wave(Al, n, ldj, ev_d, ev_e);
    } else {
        double *Ag2 = Ag;
        if (!one_wave) sym_eig_tridiag_mt(Ag2, n, ldj, ev_d, ev_e, ev_g, ev_part);
        else sym_eig_tridiag(Ag2, n, ldj, ev_d, ev_e, ev_g, sred);
        tridiag_ql_wave(Ag2, n, ldj, ev_d, ev_e);
    }
    for (int k = t; k < n; k += nt) evals[k] = ev_d[k];
    for (int w = t; w < n * n; w += nt) { int i = w / n, k = w - i * n; evecs[w] = As[i * ldj + k]; }
}

// spd_inverse_wave16 by wavefront 0 of a be_marg-sized workgroup; Ainv stays NaN where the routine does not write it
__global__ __launch_bounds__(512) void be_stage_spd_inv_kernel(int n, double floor, const double *A, double *Ainv, int *ok) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ double Al[256], L[256], Li[256], Ai[256];
    for (int w = t; w < 256; w += nt) { Al[w] = w < n * n ? A[w] : 0.0; Ai[w] = nan(""); }
    __syncthreads();
    if (t < 64) { const bool okc = spd_inverse_wave16(Al, n, floor, L, Li, Ai); if (t == 0) *ok = okc ? 1 : 0; }
    __syncthreads();
    for (int w = t; w < n * n; w += nt) Ainv[w] = Ai[w];
}

// block_scan_flags with one thread late (skew & 3: 1 = thread 0, 2 = the last thread, a few microseconds of wall_clock64 as PH() costs in the timers
// build), the flags written just before by other threads behind a barrier as the callers do (skew & 4: thread t writes the flags k = nt - 1 - t
// mod nt, all of them in other threads' chunks), and two scans back to back on the same scratch (skew & 8: the second result goes to offs + n).
// The scratch words beyond the 2 nt + 2 the routine may use are guards; guard_ok = 0 if one changed.
#define SCAN_GUARDS 16
__global__ __launch_bounds__(1024) void be_stage_scan_kernel(int n, int skew, const int *src, int *flags, int *offs, int *total, int *guard_ok) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ int scratch[2 * 1024 + 2 + SCAN_GUARDS];
    const int g0 = 2 * nt + 2;
    for (int k = t; k < SCAN_GUARDS; k += nt) scratch[g0 + k] = 0x5ca1ab1e ^ k;
    if (skew & 4) {
        for (int k = nt - 1 - t; k < n; k += nt) flags[k] = src[k];
        __syncthreads();
    }
    const bool late = ((skew & 3) == 1 && t == 0) || ((skew & 3) == 2 && t == nt - 1);
    if (late) { const long long c0 = (long long)wall_clock64(); while ((long long)wall_clock64() - c0 < 500) {} }
    const int tot = block_scan_flags(flags, n, offs, scratch);
    int tot2 = tot;
    if (skew & 8) {
        if (late) { const long long c0 = (long long)wall_clock64(); while ((long long)wall_clock64() - c0 < 500) {} }
        tot2 = block_scan_flags(flags, n, offs + n, scratch);
    }
    if (t == 0) { total[0] = tot; total[1] = tot2; }
    __syncthreads();
    if (t == 0) {
        int good = 1;
        for (int k = 0; k < SCAN_GUARDS; k++) if (scratch[g0 + k] != (0x5ca1ab1e ^ k)) good = 0;
        *guard_ok = good;
    }
}

// chol_blocked + chol_solve_blocked on a matrix in HBM (be_solve when the Schur complement does not fit LDS), 16 x 16 diagonal block in LDS as there
__global__ __launch_bounds__(1024) void be_stage_chol_blocked_kernel(int n, double *A, const double *rhs, double *xout) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ double Lpp[256];
    __shared__ int flag;
    extern __shared__ __attribute__((aligned(16))) double cb_xs[];
    for (int q = t; q < n; q += nt) cb_xs[q] = rhs[q];
    __syncthreads();
    const bool ok = chol_blocked(A, n, n, &flag, Lpp);
    if (ok) chol_solve_blocked(A, n, n, cb_xs, Lpp);
    __syncthreads();
    for (int q = t; q < n; q += nt) xout[q] = ok ? cb_xs[q] : nan("");
}
}  // namespace

// dynamic LDS the kernel can still get: the per-block maximum less its static arrays
static int stage_lds_cap(const void *kernel) {
    int cap = 0, dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || cap <= 0) cap = 64 * 1024;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) return 0;
    return cap - (int)fa.sharedSizeBytes;
}

extern "C" int vio_stage_jacobi(int mode, int n, int nt, const double *A, double *evals, double *evecs, int *sweeps_out) {
    if (mode < 0 || mode > 3 || n < 1 || !A || !evals || !evecs || nt < 64 || nt > 1024 || (nt & 63)) return VIO_EINVAL;
    if ((mode == 0 || mode == 2) && n > 16) return VIO_EINVAL;
    if (n > JAC_HBM_MAX) return VIO_EINVAL;
    const bool hbm = mode == 3 || (mode == 1 && n > JAC_LDS_MAX);
    int hs = 0;
    const size_t nn = (size_t)n * n, lds = hbm ? 0 : 2 * nn * sizeof(double);
    DevBuf<double> dA, dV;
    DevBuf<int> ds;
    std::vector<double> hA(nn);
    if ((long)lds > (long)stage_lds_cap((const void *)be_stage_jacobi_kernel)) return VIO_EINVAL;
    HIPCHK(dA.alloc(nn)); HIPCHK(dV.alloc(nn)); HIPCHK(ds.alloc(1));
    HIPCHK(dA.upload(A, nn));
    if (lds) HIPCHK(hipFuncSetAttribute((const void *)be_stage_jacobi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    be_stage_jacobi_kernel<<<1, nt, lds>>>(mode, n, dA, dV, ds);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dA.download(hA.data(), nn)); HIPCHK(dV.download(evecs, nn));
    HIPCHK(ds.download(&hs, 1));
    for (int k = 0; k < n; k++) evals[k] = hA[(size_t)k * n + k];
    if (sweeps_out) *sweeps_out = mode == 0 ? 0 : hs;
    return VIO_OK;
}

extern "C" int vio_stage_sym_eig_lds(int n, int one_wave, int in_hbm, const double *A, double *evals, double *evecs) {
    if (n < 1 || n > 128 || !A || !evals || !evecs) return VIO_EINVAL;
    const size_t nn = (size_t)n * n, lds = in_hbm ? 0 : (size_t)n * (n | 1) * sizeof(double);
    DevBuf<double> dA, dG, dw, dV;
    HIPCHK(dA.alloc(nn)); HIPCHK(dG.alloc(nn)); HIPCHK(dw.alloc((size_t)n));
    HIPCHK(dV.alloc(nn));
    HIPCHK(dA.upload(A, nn));
    if (lds) HIPCHK(hipFuncSetAttribute((const void *)be_stage_sym_eig_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    be_stage_sym_eig_lds_kernel<<<1, 512, lds>>>(n, one_wave ? 1 : 0, in_hbm ? 1 : 0, dA, dG, dw, dV);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dw.download(evals, (size_t)n)); HIPCHK(dV.download(evecs, nn));
    return VIO_OK;
}

extern "C" int vio_stage_spd_inverse16(int n, double floor, const double *A, double *Ainv, int *ok_out) {
    if (n < 1 || n > 16 || !A || !Ainv || !ok_out) return VIO_EINVAL;
    const size_t nn = (size_t)n * n;
    DevBuf<double> dA, dI;
    DevBuf<int> dok;
    HIPCHK(dA.alloc(nn)); HIPCHK(dI.alloc(nn)); HIPCHK(dok.alloc(1));
    HIPCHK(dA.upload(A, nn));
    be_stage_spd_inv_kernel<<<1, 512>>>(n, floor, dA, dI, dok);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dI.download(Ainv, nn)); HIPCHK(dok.download(ok_out, 1));
    return VIO_OK;
}

extern "C" int vio_stage_scan_flags(int n, int nt, int skew, const int *flags, int *offs, int *total_out) {
    if (n < 0 || n > (1 << 20) || nt < 64 || nt > 1024 || (nt & 63) || skew < 0 || skew > 15 || (n > 0 && (!flags || !offs)) || !total_out) return VIO_EINVAL;
    const size_t nb = (size_t)(n > 0 ? n : 1);
    const int nout = (skew & 8) ? 2 : 1;
    DevBuf<int> dsrc, dfl, doffs, dtot;
    int htot[3] = {0, 0, 0};
    HIPCHK(dsrc.alloc(nb)); HIPCHK(dfl.alloc(nb)); HIPCHK(doffs.alloc(nb * nout));
    HIPCHK(dtot.alloc(3));
    if (n > 0) {
        HIPCHK(dsrc.upload(flags, (size_t)n));
        if (skew & 4) HIPCHK(hipMemset(dfl, 0xff, (size_t)n * 4));   // (whatever the flags held before the writers ran)
        else HIPCHK(dfl.upload(flags, (size_t)n));
    }
    be_stage_scan_kernel<<<1, nt>>>(n, skew, dsrc, dfl, doffs, dtot, dtot + 2);
    HIPCHK(hipDeviceSynchronize());
    if (n > 0) HIPCHK(doffs.download(offs, (size_t)n * nout));
    HIPCHK(dtot.download(htot, 3));
    total_out[0] = htot[0]; total_out[1] = htot[1]; total_out[2] = htot[2];
    return VIO_OK;
}

// blocks = -8 / -9 of vio_stage_chol: chol_blocked + chol_solve_blocked at be_solve_kernel's 1024 / be_solve_kernel_512's 512 threads
static int stage_chol_blocked(int nb, int nt, const double *S, const double *rhs, double *L_out, double *x_out) {
    const size_t n = 16 * (size_t)nb;
    DevBuf<double> dA, dr, dx;
    std::vector<double> hA(n * n);
    HIPCHK(dA.alloc(n * n)); HIPCHK(dr.alloc(n)); HIPCHK(dx.alloc(n));
    HIPCHK(dA.upload(S, n * n)); HIPCHK(dr.upload(rhs, n));
    be_stage_chol_blocked_kernel<<<1, nt, n * sizeof(double)>>>((int)n, dA, dr, dx);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dA.download(hA.data(), n * n)); HIPCHK(dx.download(x_out, n));
    for (size_t i = 0; i < n; i++) for (size_t j = 0; j <= i; j++) L_out[i * n + j] = hA[i * n + j];
    return VIO_OK;
}

// ---- the landmark Schur complement (be_solve, solve_mode 0) and be_marg's truncated pseudo-inverse
#define SCHUR_GUARDS 64
namespace {
// variant 0: schur_mfma into S in HBM; 1: schur_mfma_lds, 2: schur_mfma_staged<9> into the LDS tile region of be_solve's size (ntile * 256 doubles),
// followed by SCHUR_GUARDS guard words; the lower tiles are untiled into S on the way out
__global__ __launch_bounds__(1024) void be_stage_schur_kernel(int variant, int n, int Kpad, unsigned colmask, const double *H, const double *Ws, const double *inv,
                                                              const double *dgp, const double *sp, double mu, double *S, int *guard_ok) {
    extern __shared__ __attribute__((aligned(16))) double sc_T[];
    const int t = threadIdx.x, nt = blockDim.x, nb = n >> 4, ntile = nb * (nb + 1) / 2;
    const double gval = -1.2345678901234567e300;
    if (variant == 0) { schur_mfma(H, Ws, inv, dgp, sp, mu, Kpad, n, n, S); if (t == 0) *guard_ok = 1; return; }
    double *guard = sc_T + (size_t)ntile * 256;
    for (int q = t; q < SCHUR_GUARDS; q += nt) guard[q] = gval;
    __syncthreads();
    if (variant == 1) schur_mfma_lds(H, Ws, inv, dgp, sp, mu, Kpad, n, n, sc_T);
    else schur_mfma_staged<9>(H, Ws, inv, dgp, sp, mu, Kpad, n, n, sc_T, colmask);
    for (int q = t; q < ntile * 256; q += nt) {
        int ti, tj;
        tri_decode(q >> 8, ti, tj);
        const int r = (q >> 4) & 15, c = q & 15;
        S[(size_t)(16 * ti + r) * n + 16 * tj + c] = sc_T[tl_idx(ti, tj, r, c)];
    }
    __syncthreads();
    if (t == 0) {
        int good = 1;
        for (int q = 0; q < SCHUR_GUARDS; q++) if (guard[q] != gval) good = 0;
        *guard_ok = good;
    }
}

// marg_pinv15 as be_marg calls it (512 threads, the same LDS arrays)
__global__ __launch_bounds__(512) void be_stage_pinv15_kernel(int md, const double *A, double *Pout, int *path) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ double cs[VIO_MAXW * 3 + 10], sn[VIO_MAXW * 3 + 10];
    __shared__ int pp[VIO_MAXW * 3 + 10], qq[VIO_MAXW * 3 + 10];
    __shared__ double A15[225], V15[225], Pinv[225], L15[225], Am[225];
    __shared__ int pinv_direct;
    for (int w = t; w < md * md; w += nt) Am[w] = A[w];
    __syncthreads();
    marg_pinv15(Am, md, md, 1e-8, A15, V15, L15, Pinv, cs, sn, pp, qq, &pinv_direct);
    for (int w = t; w < md * md; w += nt) Pout[w] = Pinv[w];
    if (t == 0) *path = pinv_direct ? 0 : 1;
}
}  // namespace

extern "C" int vio_stage_schur(int variant, int nb, int nt, int Kpad, unsigned colmask, const double *H, const double *Ws, const double *inv, const double *dgp,
                               const double *sp, double mu, double *S_out, int *guard_ok) {
    if (variant < 0 || variant > 2 || nb < 1 || nb > VIO_LWMAX / 16 || nt < 64 || nt > 1024 || (nt & 63) || Kpad < 0 || (Kpad & 3) || Kpad > 4096 ||
        !H || !S_out || !guard_ok || !dgp || !sp || (Kpad > 0 && (!Ws || !inv)))
        return VIO_EINVAL;
    const int n = 16 * nb, ntile = nb * (nb + 1) / 2;
    if (variant >= 1 && ntile * 256 > 16896) return VIO_EINVAL;                  // be_solve's tiles_in_lds
    if (variant == 2 && !schur_staged_ok(n, nt)) return VIO_EINVAL;
    int hg = 0;
    const size_t nn = (size_t)n * n, kw = (size_t)(Kpad > 0 ? Kpad : 1) * n, lds = variant ? ((size_t)ntile * 256 + SCHUR_GUARDS) * sizeof(double) : 0;
    DevBuf<double> dH, dW, di, dd, ds, dS;
    DevBuf<int> dg;
    HIPCHK(dH.alloc(nn)); HIPCHK(dW.alloc(kw)); HIPCHK(di.alloc((size_t)Kpad + 1));
    HIPCHK(dd.alloc((size_t)n)); HIPCHK(ds.alloc((size_t)n)); HIPCHK(dS.alloc(nn));
    HIPCHK(dg.alloc(1));
    HIPCHK(dH.upload(H, nn)); HIPCHK(dS.upload(S_out, nn));
    if (Kpad > 0) { HIPCHK(dW.upload(Ws, (size_t)Kpad * n)); HIPCHK(di.upload(inv, (size_t)Kpad)); }
    HIPCHK(dd.upload(dgp, (size_t)n)); HIPCHK(ds.upload(sp, (size_t)n));
    if (lds) HIPCHK(hipFuncSetAttribute((const void *)be_stage_schur_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    be_stage_schur_kernel<<<1, nt, lds>>>(variant, n, Kpad, colmask, dH, dW, di, dd, ds, mu, dS, dg);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dS.download(S_out, nn)); HIPCHK(dg.download(&hg, 1));
    *guard_ok = hg;
    return VIO_OK;
}

extern "C" int vio_stage_pinv15(int n, const double *A, double *Pinv, int *path_out) {
    if (n < 1 || n > 15 || !A || !Pinv || !path_out) return VIO_EINVAL;
    const size_t nn = (size_t)n * n;
    DevBuf<double> dA, dP;
    DevBuf<int> dp;
    HIPCHK(dA.alloc(nn)); HIPCHK(dP.alloc(nn)); HIPCHK(dp.alloc(1));
    HIPCHK(dA.upload(A, nn));
    be_stage_pinv15_kernel<<<1, 512>>>(n, dA, dP, dp);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dP.download(Pinv, nn)); HIPCHK(dp.download(path_out, 1));
    return VIO_OK;
}
