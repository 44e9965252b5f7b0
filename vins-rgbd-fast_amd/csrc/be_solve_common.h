// What the persistent solver and the marginalisation (be_kernels.hip) and the phased solver (be_phased.h) share: landmark
// compaction, the prior's dx, frame-pair geometry staging, the packed pair-block indexing, landmark rows, the IMU Gram block on the
// matrix cores, and everything optimization() does before the first and after the last evaluation (solve_prologue / solve_epilogue).
#pragma once
#include "be_ctx.h"
#include "be_linalg.h"
#include "be_preint.h"

namespace {

// 4x4 / small symmetric cyclic Jacobi (row-cyclic, as oracle/om.h sym_eig); A destroyed, eigenvalues unsorted in A diag
// stable compaction of the landmark order list; flags[k] = keep. Freed slots go back to the free stack.
__device__ void lm_compact(Ctx &c, int *flags, int *offs, int *scratch) {
    int n = c.be->n_lm;
    int kept = block_scan_flags(flags, n, offs, scratch);
    const int t = threadIdx.x, nt = blockDim.x;
    int nfree0 = c.be->n_free;
    for (int k = t; k < n; k += nt) c.lm_tmp[k] = c.lm_order[k];
    __syncthreads();
    for (int k = t; k < n; k += nt) {
        int slot = c.lm_tmp[k];
        if (flags[k]) c.lm_order[offs[k]] = slot;
        else c.lm_free[nfree0 + (k - offs[k])] = slot;
    }
    __syncthreads();
    if (t == 0) { c.be->n_lm = kept; c.be->n_free = nfree0 + (n - kept); }
    __syncthreads();
}

// the same compaction on LDS copies of the order list, the flags and the offsets (finish_body<true>): the counters stay in registers (n, nfree:
// uniform over the workgroup), the freed slots go to the free stack in HBM in the same places; the caller writes order / counters back once
__device__ void lm_compact_staged(Ctx &c, int *ord, int *tmp, int *flags, int *offs, int *scratch, int &n, int &nfree) {
    const int kept = block_scan_flags(flags, n, offs, scratch);
    const int t = threadIdx.x, nt = blockDim.x;
    for (int k = t; k < n; k += nt) tmp[k] = ord[k];
    __syncthreads();
    // (two loops: as one if / else the compiler merges the two stores into a single flat store through a selected LDS-or-HBM address)
    for (int k = t; k < n; k += nt) if (flags[k]) ord[offs[k]] = tmp[k];
    for (int k = t; k < n; k += nt) if (!flags[k]) c.lm_free[nfree + (k - offs[k])] = tmp[k];
    __syncthreads();
    nfree += n - kept;
    n = kept;
}

// pre_integrations[j]->repropagate(Vector3d::Zero(), Bgs[j]) for every window slot (estimator.cpp:275-279, :829-836), block-cooperative
__device__ void repropagate_window(Ctx &c, PreWork &pw) {
    const int t = threadIdx.x, nt = blockDim.x, W = c.W;
    BeSeq &be = *c.be;
    const vio_config &cfg = c.C->c;
    for (int j = 0; j <= W; j++) {
            PreInt &p = c.pre[be.pre_idx[j]];
            if (!p.valid) continue;
            if (t == 0) {
                int nb = p.n_buf;
                v3 la = ld3(p.lin_acc), lg = ld3(p.lin_gyr);
                p.sum_dt = 0;
                st3(p.acc0, la); st3(p.gyr0, lg);
                p.dp[0] = p.dp[1] = p.dp[2] = 0; p.dv[0] = p.dv[1] = p.dv[2] = 0;
                p.dq[0] = 1; p.dq[1] = p.dq[2] = p.dq[3] = 0;
                p.lin_ba[0] = p.lin_ba[1] = p.lin_ba[2] = 0;
                st3(p.lin_bg, ld3(be.Bgs[j]));
                p.n_buf = nb;
            }
            for (int i = t; i < 225; i += nt) { pw.J[i] = ((i / 15) == (i % 15)) ? 1.0 : 0.0; pw.Pm[i] = 0; }
            __syncthreads();
            for (int q = 0; q < p.n_buf; q++) preint_propagate(p, pw, *c.K, p.dt_buf[q], ld3(p.acc_buf[q]), ld3(p.gyr_buf[q]));
            preint_store(p, pw);
        }
}

// prior residual row i at parameters X: r0 + J dx; dx assembled in LDS sdx (n)
__device__ __forceinline__ void prior_dx(const Ctx &c, const Params &X, double *sdx, bool sync = true) {
    const int t = threadIdx.x, W = c.W;
    const BeSeq &be = *c.be;
    if (t <= W + 2) {
        if (t < W) {
            double d[6];
            bf::pose_dx(&X.pose[t * 7], &c.prior_x0[t * 7], d);
            for (int k = 0; k < 6; k++) sdx[6 * t + k] = be.prior_present[t] ? d[k] : 0.0;
        } else if (t == W) {
            for (int k = 0; k < 9; k++) sdx[6 * W + k] = be.prior_present[W] ? X.sb[k] - c.prior_x0[W * 7 + k] : 0.0;
        } else if (t == W + 1) {
            double d[6];
            bf::pose_dx(X.ex, &c.prior_x0[W * 7 + 9], d);
            for (int k = 0; k < 6; k++) sdx[6 * W + 9 + k] = be.prior_present[W + 1] ? d[k] : 0.0;
        } else
            sdx[6 * W + 15] = be.prior_present[W + 2] ? X.td - c.prior_x0[W * 7 + 16] : 0.0;
    }
    if (sync) __syncthreads();
}
// tangent index of prior slot a
__device__ __forceinline__ int prior_map(int a, int W) {
    if (a < 6 * W) return a;                                  // pose k at 6k
    if (a < 6 * W + 9) return 6 * (W + 1) + (a - 6 * W);     // speed-bias 0
    if (a < 6 * W + 15) return 15 * (W + 1) + (a - 6 * W - 9);
    return 15 * (W + 1) + 6;
}

// Frame-pair geometry of the evaluation point X: a table of 32-double records (be_factors.h PairGeo: A1, A2, M, t) and, as record nrec, ric.
// The one place that fills such a table; the callers differ in how a record is indexed only: pair(p, i, j) names the frames of record p and
// says whether the record is wanted (a pair without residuals is left as it is).  Called by every thread of the workgroup (nt of them); ends
// with the barrier behind which the table may be read.
template <class Pair>
__device__ __forceinline__ void stage_pair_geo(const Params &X, double *geo, const int nrec, const int nt, Pair pair) {
    for (int p = threadIdx.x; p <= nrec; p += nt) {
        if (p == nrec) { stm(geo + (size_t)p * 32, q2R(mkq(X.ex[6], X.ex[3], X.ex[4], X.ex[5]))); continue; }
        int i, j;
        if (!pair(p, i, j)) continue;
        bf::PairGeo g;
        bf::pair_geo(&X.pose[i * 7], &X.pose[j * 7], X.ex, g);
        double *o = geo + (size_t)p * 32;
        for (int q = 0; q < 9; q++) { o[q] = g.A1[q]; o[9 + q] = g.A2[q]; o[18 + q] = g.M[q]; }
        o[27] = g.t[0]; o[28] = g.t[1]; o[29] = g.t[2];
    }
    __syncthreads();
}
// record p = i W1 + j of the square table (be_solve's evaluate, ps_eval): the pairs i < j that have residuals
__device__ __forceinline__ bool pair_of_square(const Ctx &c, const int W1, const int p, int &i, int &j) {
    i = p / W1; j = p - i * W1;
    return i < j && c.pair_start[p + 1] != c.pair_start[p];
}
// where a projection record keeps its weighted residual: behind the two Jacobian rows of the 42-double layout (vext, relocalisation), in
// the last column of each row of the compact 28-double one
__device__ __forceinline__ void rec_put_wr(double *out, const bool compact, const double wgt, const double *rr) {
    out[compact ? 13 : 40] = wgt * rr[0];
    out[compact ? 27 : 41] = wgt * rr[1];
}

// pair-block entry index of the packed symmetric 20x20
__device__ __forceinline__ int sym_idx(int a, int b) {
    if (a > b) { int x = a; a = b; b = x; }
    return a * 20 - a * (a - 1) / 2 + (b - a);
}
__device__ __forceinline__ int local_of(int a, int i, int j, int W) {
    // tangent index a within the vision set -> local column of pair (i,j) or -1
    int np = 6 * (W + 1);
    if (a < np) {
        int f = a / 6, d = a - f * 6;
        if (f == i) return d;
        if (f == j) return 6 + d;
        return -1;
    }
    int e = a - 15 * (W + 1);
    return 12 + e;  // ex 0..5 -> 12..17, td (6) -> 18
}

#define PB_U 8  // k groups (of 4 Jacobian rows) loaded per batch in the frame-pair block phase of assemble
// compact index of the frame pair (i < j)
__device__ __forceinline__ int pair_slot(int i, int j, int W1) { return i * W1 - i * (i + 1) / 2 + (j - i - 1); }

// One half of a landmark's coupling row (see assemble): `res` = the landmark's residual Jacobians (42 doubles each, observation k
// at res + 42 (k - 1)), `row` = its Hpl row.  The arrays never overlap; the restrict qualifiers let the loads of the next
// residual be issued ahead of the row stores of the current one (the loop is bound by the latency of those loads).
__device__ __forceinline__ void lm_row(const double *__restrict__ res, double *__restrict__ row, double *__restrict__ Hll,
                                       double *__restrict__ gl, int half, int st, int kend, int ext_off, int krelo = -1) {
    // krelo: index of the landmark's relocalisation record (rides behind the regular ones, be_phased.h) or -1.  Its pose_j group is
    // zero by construction and it has no frame st + k of its own: no pose_j store for it (which would land on whatever columns follow)
    // residual records are 336 bytes apart and 16-byte aligned: 16-byte loads halve the number of cache-line lookups of this gather
    if (half == 0) {
        double si[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 2
        for (int k = 1; k < kend; k++) {
            const double *Jr = res + (size_t)(k - 1) * 42;
            const double2 *J2 = (const double2 *)Jr;
            const double l0 = Jr[19], l1 = Jr[39];
            double a[6], b[6], e[6], f[6];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double2 va = J2[q], vb = J2[3 + q], ve = J2[10 + q], vf = J2[13 + q];
                a[2 * q] = va.x; a[2 * q + 1] = va.y; b[2 * q] = vb.x; b[2 * q + 1] = vb.y;
                e[2 * q] = ve.x; e[2 * q + 1] = ve.y; f[2 * q] = vf.x; f[2 * q + 1] = vf.y;
            }
#pragma unroll
            for (int d = 0; d < 6; d++) {
                si[d] += a[d] * l0 + e[d] * l1;
                if (k != krelo) row[6 * (st + k) + d] = b[d] * l0 + f[d] * l1;
            }
        }
#pragma unroll
        for (int d = 0; d < 6; d++) row[6 * st + d] = si[d];
    } else {
        double se[7] = {0, 0, 0, 0, 0, 0, 0}, hll = 0, gg = 0;
#pragma unroll 2
        for (int k = 1; k < kend; k++) {
            const double *Jr = res + (size_t)(k - 1) * 42;
            const double2 *J2 = (const double2 *)Jr;
            double a[8], e[8];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double2 va = J2[6 + q], ve = J2[16 + q];   // Jr[12..19], Jr[32..39]
                a[2 * q] = va.x; a[2 * q + 1] = va.y; e[2 * q] = ve.x; e[2 * q + 1] = ve.y;
            }
            const double2 rr = J2[20];                      // weighted residual (Jr[40], Jr[41])
            const double l0 = a[7], l1 = e[7];
#pragma unroll
            for (int d = 0; d < 7; d++) se[d] += a[d] * l0 + e[d] * l1;
            hll += l0 * l0 + l1 * l1;
            gg += l0 * rr.x + l1 * rr.y;
        }
#pragma unroll
        for (int d = 0; d < 7; d++) row[ext_off + d] = se[d];
        *Hll = hll;
        *gl = gg;
    }
}

// IMU factor block on the FP64 matrix cores (one wavefront): raw_l = [J_raw | r_whitened] (15 x 31, LDS), M_l = chol(cov)^-1 (15 x 15
// lower triangular, LDS).  The rows of J are whitened on the fly (x = M J_raw, one output row per lane group) and the 31 x 31 Gram
// matrix [Jw r]^T [Jw r] is accumulated with K = 16 (row 15 is padding): a00 = rows / cols 0-15, a10 = rows 16-31 x cols 0-15,
// a11 = rows / cols 16-31, in the C/D layout of v_mfma_f64_16x16x4_f64 (element r of lane (lk, li) = row lk + 4 r, column li).
__device__ __forceinline__ void imu_block_mfma(const double *raw_l, const double *M_l, int li, int lk, v4f64 &a00, v4f64 &a10, v4f64 &a11) {
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        const int kk = 4 * ks + lk;
        double x0 = 0, x1 = 0;
        if (kk < 15) {
            const int c1 = 16 + li;
            for (int k = 0; k <= kk; k++) {
                double m = M_l[kk * 15 + k];
                x0 += m * raw_l[k * 31 + li];
                if (c1 < 30) x1 += m * raw_l[k * 31 + c1];
            }
            if (c1 == 30) x1 = raw_l[kk * 31 + 30];
        }
        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, a00, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, a11, 0, 0, 0);
    }
}

// The same for the compact residual records (28 doubles, no extrinsic / td columns): half 0 = pose columns, half 1 = Hll and gl.
__device__ __forceinline__ void lm_row_compact(const double *__restrict__ res, double *__restrict__ row, double *__restrict__ Hll,
                                               double *__restrict__ gl, int half, int st, int kend) {
    if (half == 0) {
        double si[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 2
        for (int k = 1; k < kend; k++) {
            const double2 *J2 = (const double2 *)(res + (size_t)(k - 1) * 28);
            double a[6], b[6], e[6], f[6];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double2 va = J2[q], vb = J2[3 + q], ve = J2[7 + q], vf = J2[10 + q];
                a[2 * q] = va.x; a[2 * q + 1] = va.y; b[2 * q] = vb.x; b[2 * q + 1] = vb.y;
                e[2 * q] = ve.x; e[2 * q + 1] = ve.y; f[2 * q] = vf.x; f[2 * q + 1] = vf.y;
            }
            const double l0 = J2[6].x, l1 = J2[13].x;
#pragma unroll
            for (int d = 0; d < 6; d++) {
                si[d] += a[d] * l0 + e[d] * l1;
                row[6 * (st + k) + d] = b[d] * l0 + f[d] * l1;
            }
        }
#pragma unroll
        for (int d = 0; d < 6; d++) row[6 * st + d] = si[d];
    } else {
        double hll = 0, gg = 0;
#pragma unroll 2
        for (int k = 1; k < kend; k++) {
            const double2 *J2 = (const double2 *)(res + (size_t)(k - 1) * 28);
            const double2 p0 = J2[6], p1 = J2[13];   // (inv_depth column, weighted residual) of the two rows
            hll += p0.x * p0.x + p1.x * p1.x;
            gg += p0.x * p0.y + p1.x * p1.y;
        }
        *Hll = hll;
        *gl = gg;
    }
}

// Everything optimization() does before the first evaluation (estimator.cpp:1161-1212, 936-981): static-initialisation extras,
// vector2double into X, landmark / residual / frame-pair indexing, constness decisions (sh_i[0] = extrinsic variable, sh_i[1] = td
// variable).  Shared by the persistent solve kernel and the phased solver (ps_setup_kernel).
// allow_relo: the caller can carry relocalisation factors (phased solver): sh_i[4] returns whether this solve has them
__device__ __forceinline__ void solve_prologue(const Batch &B, Ctx &c, Params &X, int *scratch, PreWork &pw, int *sh_i, int &F, int &Fa, int &nres,
                                               const bool allow_relo = false, unsigned *lmkey = nullptr, const int lmkey_cap = 0) {
    const int t = threadIdx.x, nt = blockDim.x;
    const vio_config &cfg = c.C->c;
    BeSeq &be = *c.be;
    const int W = c.W, W1 = W + 1;
    const int s = c.s;
    PH_INIT;
    // ---- static initialisation extras (estimator.cpp:266-283): solveGyroscopeBias + repropagate (IMU mode only, :264)
    if (be.solver_flag == 0 && cfg.use_imu) {
        if (t == 0) {
            double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
            for (int i = 0; i < W; i++) {
                int j = i + 1;
                const PreInt &p = c.pre[be.pre_idx[j]];
                quat q_ij = R2q(mul(tr(ldm(be.Rs[i])), ldm(be.Rs[j])));
                m3 tA = bf::get33(p.jac, 15, bf::O_R, bf::O_BG);
                v3 tb = scl(2.0, qvec(qmul(qinv(mkq(p.dq[0], p.dq[1], p.dq[2], p.dq[3])), q_ij)));
                m3 AtA = mul(tr(tA), tA);
                v3 Atb = mul(tr(tA), tb);
                for (int r = 0; r < 9; r++) A[r] += AtA.a[r];
                b[0] += Atb.x; b[1] += Atb.y; b[2] += Atb.z;
            }
            double M[12];
            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) M[r * 4 + q] = A[r * 3 + q]; M[r * 4 + 3] = b[r]; }
            for (int i = 0; i < 3; i++) {
                int p = i;
                for (int r = i + 1; r < 3; r++) if (fabs(M[r * 4 + i]) > fabs(M[p * 4 + i])) p = r;
                for (int q = 0; q < 4; q++) { double tmp = M[i * 4 + q]; M[i * 4 + q] = M[p * 4 + q]; M[p * 4 + q] = tmp; }
                if (M[i * 4 + i] == 0) continue;
                for (int r = i + 1; r < 3; r++) {
                    double f = M[r * 4 + i] / M[i * 4 + i];
                    for (int q = i; q < 4; q++) M[r * 4 + q] -= f * M[i * 4 + q];
                }
            }
            double x[3] = {0, 0, 0};
            for (int i = 2; i >= 0; i--) {
                double sacc = M[i * 4 + 3];
                for (int q = i + 1; q < 3; q++) sacc -= M[i * 4 + q] * x[q];
                x[i] = M[i * 4 + i] != 0 ? sacc / M[i * 4 + i] : 0;
            }
            for (int i = 0; i <= W; i++) { be.Bgs[i][0] += x[0]; be.Bgs[i][1] += x[1]; be.Bgs[i][2] += x[2]; }
        }
        __syncthreads();
        repropagate_window(c, pw);
    }

    // ---- vector2double (estimator.cpp:936-981)
    if (t <= W) {
        int i = t;
        X.pose[i * 7 + 0] = be.Ps[i][0]; X.pose[i * 7 + 1] = be.Ps[i][1]; X.pose[i * 7 + 2] = be.Ps[i][2];
        quat q = R2q(ldm(be.Rs[i]));
        X.pose[i * 7 + 3] = q.x; X.pose[i * 7 + 4] = q.y; X.pose[i * 7 + 5] = q.z; X.pose[i * 7 + 6] = q.w;
        for (int k = 0; k < 3; k++) { X.sb[i * 9 + k] = be.Vs[i][k]; X.sb[i * 9 + 3 + k] = be.Bas[i][k]; X.sb[i * 9 + 6 + k] = be.Bgs[i][k]; }
    }
    if (t == W + 1) {
        X.ex[0] = be.tic[0]; X.ex[1] = be.tic[1]; X.ex[2] = be.tic[2];
        quat q = R2q(ldm(be.ric));
        X.ex[3] = q.x; X.ex[4] = q.y; X.ex[5] = q.z; X.ex[6] = q.w;
        X.td = be.td;
        for (int k = 0; k < 7; k++) X.relo[k] = be.relo_Pose[k];
    }
    // constness (estimator.cpp:1187-1212), decided first because the relocalisation factors borrow the columns of a CONSTANT extrinsic
    if (t == 0) {
        double v0 = nrm(ld3(be.Vs[0]));
        int ex_active;
        if ((cfg.estimate_extrinsic && be.frame_count == W && v0 > 0.2) || be.openExEstimation) { be.openExEstimation = 1; ex_active = 1; }
        else ex_active = 0;
        int td_active = cfg.use_imu && cfg.estimate_td && !(v0 < 0.2);   // no td block without the IMU (estimator.cpp:1204)
        sh_i[0] = ex_active; sh_i[1] = td_active;
        // (no solver_flag test, like optimization(): the solve that ends the static initialisation runs with solver_flag still 0 here, and
        // solve_epilogue consumes the request after it)
        int relo_on = be.relo_info;
        if (relo_on && (!allow_relo || !cfg.use_imu)) {
            // relocalisation on the persistent solver (windows beyond the phased solver's range) and in VO mode (solve_epilogue's VO branch
            // neither moves relo_Pose nor consumes the request) is not supported: the request is dropped and the frame flagged (overflow
            // bit 64); optimization() without relocalization_info is what runs
            relo_on = 0; be.relo_info = 0; be.overflow |= 64;
        } else if (relo_on && ex_active) {
            // DEVIATION 15: relo_Pose borrows the six tangent columns of the extrinsic in the reduced system, so the extrinsic is held constant
            // in the (one) solve that carries relocalisation factors even when ESTIMATE_EXTRINSIC has opened it; openExEstimation stays
            // latched and the next solve refines it again.  The oracle mirrors this under reference_quirks bit 2 (tests).
            ex_active = 0; sh_i[0] = 0;
        }
        sh_i[4] = relo_on; sh_i[3] = 0;
    }
    __syncthreads();
    const int relo_on = sh_i[4];
    PH(100);
    // ---- landmark indexing: in-problem (para_Feature index), variable landmarks, residual list
    const int nlm = be.n_lm;
    int *tmpA = c.pair_list, *tmpB = c.pair_list + c.NL;       // scan temporaries (pair_list proper is built afterwards)
    int *alist = c.pair_list + c.nres_cap - c.NL;              // variable-landmark slots, kept for the whole solve
    int *plist = c.pair_list + c.nres_cap - 2 * c.NL;          // in-problem landmark slots in list order
    __syncthreads();
    for (int k = t; k < nlm; k += nt) tmpA[k] = in_problem(c, c.lm_order[k]) ? 1 : 0;
    __syncthreads();
    F = block_scan_flags(tmpA, nlm, tmpB, scratch);
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k];
        c.lm_pidx[slot] = tmpA[k] ? tmpB[k] : -1;
        if (tmpA[k]) { c.feat[tmpB[k]] = 1.0 / c.lm_depth[slot]; plist[tmpB[k]] = slot; }
    }
    __syncthreads();
    // variable landmarks (not SetParameterBlockConstant): estimator.cpp:1278-1298
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k];
        tmpA[k] = (c.lm_pidx[slot] >= 0 && !(c.lm_est[slot] == 1 && cfg.fix_depth)) ? 1 : 0;
    }
    __syncthreads();
    Fa = block_scan_flags(tmpA, nlm, tmpB, scratch);
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k];
        c.lm_aidx[slot] = tmpA[k] ? tmpB[k] : -1;
        if (tmpA[k]) alist[tmpB[k]] = slot;
    }
    __syncthreads();
    PH(101);
    // relocalisation factors (estimator.cpp:1307-1346): in-problem landmarks with start_frame <= relo_frame_local_index whose id is among
    // the match points (upstream walks both ascending lists with one cursor: the same set); their factor rides as one more residual
    // record behind the landmark's regular ones, marked res_k = 0
    for (int k = t; k < nlm; k += nt) {
        const int slot = c.lm_order[k];
        int hit = 0;
        if (relo_on && c.lm_pidx[slot] >= 0 && c.lm_start[slot] <= be.relo_local) {
            const int id = c.lm_id[slot];
            int lo = 0, hi = be.relo_nmatch - 1;
            while (lo <= hi) {
                const int mid = (lo + hi) >> 1, mi = (int)c.relo_mp[3 * mid + 2];
                if (mi == id) { hit = 1; c.relo_xy[2 * slot] = c.relo_mp[3 * mid]; c.relo_xy[2 * slot + 1] = c.relo_mp[3 * mid + 1]; break; }
                if (mi < id) lo = mid + 1; else hi = mid - 1;
            }
        }
        c.lm_relo[slot] = hit;
        if (hit) atomicAdd(&sh_i[3], 1);
    }
    // residual list: (nobs-1) residuals per in-problem landmark, list order (estimator.cpp:1243-1302)
    for (int k = t; k < nlm; k += nt) { int slot = c.lm_order[k]; tmpA[k] = c.lm_pidx[slot] >= 0 ? c.lm_nobs[slot] - 1 + c.lm_relo[slot] : 0; }
    __syncthreads();
    nres = block_scan_flags(tmpA, nlm, tmpB, scratch);
    const int nres_max = c.nres_cap - 2 * c.NL;
    if (nres > nres_max) { nres = nres_max; if (t == 0) be.overflow |= 8; }
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k];
        int r0 = tmpB[k], cnt = tmpA[k];
        c.lm_tmp[slot] = r0;  // first residual index of this landmark
        const int nreg = c.lm_nobs[slot] - 1;
        for (int q = 0; q < cnt; q++)
            if (r0 + q < nres) { c.res_lm[r0 + q] = slot; c.res_k[r0 + q] = q < nreg ? q + 1 : 0; }
    }
    __syncthreads();
    PH(102);
    // frame-pair lists in deterministic (landmark list) order: one wavefront per frame pair walks the in-problem landmarks
    {
        const int lane = t & 63, wave = t >> 6, nw = nt >> 6;
        for (int p = t; p <= W1 * W1; p += nt) c.pair_start[p] = 0;
        // (round 6) what the walks below need of a landmark -- start frame, observation count, relocalisation mark, first residual index -- packed
        // into one word of LDS per in-problem landmark: every frame pair walks the whole list twice, W1 W / 2 pairs x F / 64 trips x 2, and from HBM
        // each trip was a chain of two dependent loads (the slot, then its fields): 214 us of ps_setup at W = 20, 55 at W = 10
        const bool keys = lmkey != nullptr && F <= lmkey_cap && c.nres_cap < (1 << 19);
        if (keys)
            for (int k = t; k < F; k += nt) {
                const int slot = plist[k];
                lmkey[k] = (unsigned)c.lm_start[slot] | ((unsigned)c.lm_nobs[slot] << 6) | ((unsigned)(c.lm_relo[slot] ? 1 : 0) << 12) | ((unsigned)c.lm_tmp[slot] << 13);
            }
        __syncthreads();
        auto lm_fields = [&](int k, int &st_, int &no_, int &rl_, int &r0_) {
            if (keys) { const unsigned key = lmkey[k]; st_ = key & 63u; no_ = (key >> 6) & 63u; rl_ = (key >> 12) & 1u; r0_ = (int)(key >> 13); }
            else { const int slot = plist[k]; st_ = c.lm_start[slot]; no_ = c.lm_nobs[slot]; rl_ = c.lm_relo[slot]; r0_ = c.lm_tmp[slot]; }
        };
        for (int p = wave; p < W1 * W1; p += nw) {
            int i = p / W1, j = p - i * W1;
            if (!(i < j)) continue;
            int cnt = 0;
            for (int k0 = 0; k0 < F; k0 += 64) {
                int k = k0 + lane;
                bool hit = false;
                bool hit2 = false;   // relocalisation record: listed with the pair (start, start + 1), its pose_j columns are zero
                if (k < F) {
                    int st_, no_, rl_, r0_;
                    lm_fields(k, st_, no_, rl_, r0_);
                    hit = st_ == i && no_ > j - i && r0_ + (j - i - 1) < nres;
                    hit2 = relo_on && j == i + 1 && st_ == i && rl_ && r0_ + no_ - 1 < nres;
                }
                cnt += __popcll(__ballot(hit)) + __popcll(__ballot(hit2));
            }
            if (lane == 0) c.pair_start[p] = cnt;
        }
        __syncthreads();
        PH(103);
        {
            // exclusive prefix sum of the W1^2 counts (one thread walking them was 441 dependent loads at W = 20): chunks per thread, Hillis-Steele
            // over the chunk sums in `scratch` (2 nt ints), as block_scan_flags does
            const int np = W1 * W1, chunk = (np + nt - 1) / nt, b0 = min(np, t * chunk), e0 = min(np, b0 + chunk);
            int vals[4], sum = 0;   // chunk <= 4: np <= 441 at W = 20 needs nt >= 111
            if (chunk <= 4) {
#pragma unroll
                for (int q = 0; q < 4; q++) { vals[q] = b0 + q < e0 ? c.pair_start[b0 + q] : 0; sum += vals[q]; }
                int *cur = scratch, *nxt = scratch + nt;
                __syncthreads();
                cur[t] = sum;
                __syncthreads();
                for (int off = 1; off < nt; off <<= 1) {
                    int v = cur[t];
                    if (t >= off) v += cur[t - off];
                    nxt[t] = v;
                    __syncthreads();
                    int *tmp = cur; cur = nxt; nxt = tmp;
                }
                int o = cur[t] - sum;
#pragma unroll
                for (int q = 0; q < 4; q++) if (b0 + q < e0) { c.pair_start[b0 + q] = o; o += vals[q]; }
                if (t == nt - 1) c.pair_start[np] = cur[nt - 1];
            } else if (t == 0) {
                int acc = 0;
                for (int p = 0; p < np; p++) { int v = c.pair_start[p]; c.pair_start[p] = acc; acc += v; }
                c.pair_start[np] = acc;
            }
        }
        __syncthreads();
        for (int p = wave; p < W1 * W1; p += nw) {
            int i = p / W1, j = p - i * W1;
            if (!(i < j)) continue;
            int o = c.pair_start[p];
            for (int k0 = 0; k0 < F; k0 += 64) {
                int k = k0 + lane;
                bool hit = false;
                int r = 0;
                if (k < F) { int st_, no_, rl_, r0_; lm_fields(k, st_, no_, rl_, r0_); r = r0_ + (j - i - 1); hit = st_ == i && no_ > j - i && r < nres; }
                unsigned long long m = __ballot(hit);
                if (hit) c.pair_list[o + __popcll(m & ((1ULL << lane) - 1ULL))] = r;
                o += __popcll(m);
            }
            if (relo_on && j == i + 1)
                for (int k0 = 0; k0 < F; k0 += 64) {
                    int k = k0 + lane;
                    bool hit = false;
                    int r = 0;
                    if (k < F) { int st_, no_, rl_, r0_; lm_fields(k, st_, no_, rl_, r0_); r = r0_ + no_ - 1; hit = st_ == i && rl_ && r < nres; }
                    unsigned long long m = __ballot(hit);
                    if (hit) c.pair_list[o + __popcll(m & ((1ULL << lane) - 1ULL))] = r;
                    o += __popcll(m);
                }
        }
        __syncthreads();
    }
    PH(104);
    if (t == 0) {
        be.n_in_problem = F; be.n_var_landmarks = Fa; be.n_residuals = nres - sh_i[3];   // (f_m_cnt counts the regular factors)
        be.relo_factors = sh_i[3];
        be.iterations = 0; be.successful = 0;
    }
    __syncthreads();
}

// double2vector + setDepth + failureDetection after the solve (estimator.cpp:985-1111, feature_manager.cpp:197-223, estimator.cpp:345-353).
// sdx: >= 12 doubles of LDS scratch.  Shared by the persistent solve kernel and the phased solver (ps_final_kernel).
__device__ __forceinline__ void solve_epilogue(Ctx &c, const Params &X, double cost, int iters_done, int succ, long long ts0, double *sdx, double *sh_d, int *sh_i) {
    const int t = threadIdx.x, nt = blockDim.x;
    const vio_config &cfg = c.C->c;
    BeSeq &be = *c.be;
    const int W = c.W, nlm = be.n_lm;
    // ---- write back flat parameters + double2vector (estimator.cpp:985-1111)
    if (!cfg.use_imu) {
        // VO mode (estimator.cpp:1060-1067, 1093, 1109): poses straight from the parameters, no gauge fix, nothing else handed back
        if (t == 0) {
            be.final_cost = cost; be.iterations = iters_done; be.successful = succ;
            be.iter_total += iters_done; be.solve_total++;
            be.dbg[4] = (int)(VIO_CLOCK() - ts0);
        }
        if (t <= W) {
            const int i = t;
            for (int k = 0; k < 7; k++) be.para_Pose[i][k] = X.pose[i * 7 + k];
            stm(be.Rs[i], q2R(qnormalized(mkq(X.pose[i * 7 + 6], X.pose[i * 7 + 3], X.pose[i * 7 + 4], X.pose[i * 7 + 5]))));
            be.Ps[i][0] = X.pose[i * 7]; be.Ps[i][1] = X.pose[i * 7 + 1]; be.Ps[i][2] = X.pose[i * 7 + 2];
        }
    } else {
    if (t == 0) {
        be.final_cost = cost; be.iterations = iters_done; be.successful = succ;
        be.iter_total += iters_done; be.solve_total++;
        be.dbg[4] = (int)(VIO_CLOCK() - ts0);
        v3 origin_R0 = R2ypr(ldm(be.Rs[0]));
        v3 origin_P0 = ld3(be.Ps[0]);
        quat q0 = mkq(X.pose[6], X.pose[3], X.pose[4], X.pose[5]);
        v3 origin_R00 = R2ypr(q2R(q0));
        double y_diff = origin_R0.x - origin_R00.x;
        m3 rot_diff = ypr2R(mk(y_diff, 0, 0));
        if (fabs(fabs(origin_R0.y) - 90) < 1.0 || fabs(fabs(origin_R00.y) - 90) < 1.0) rot_diff = mul(ldm(be.Rs[0]), tr(q2R(q0)));
        sh_d[0] = 0;
        for (int q = 0; q < 9; q++) sdx[q] = rot_diff.a[q];
        sdx[9] = origin_P0.x; sdx[10] = origin_P0.y; sdx[11] = origin_P0.z;
    }
    __syncthreads();
    // para_Pose as the solve leaves it (estimator.h:139): what Estimator::setReloFrame copies into relo_Pose when no marginalisation
    // re-runs vector2double afterwards (marg_body overwrites it in that case, like optimization() does)
    if (t <= W) for (int k = 0; k < 7; k++) be.para_Pose[t][k] = X.pose[t * 7 + k];
    if (t <= W) {
        int i = t;
        m3 rot_diff = ldm(sdx);
        v3 origin_P0 = mk(sdx[9], sdx[10], sdx[11]);
        quat qi = qnormalized(mkq(X.pose[i * 7 + 6], X.pose[i * 7 + 3], X.pose[i * 7 + 4], X.pose[i * 7 + 5]));
        stm(be.Rs[i], mul(rot_diff, q2R(qi)));
        st3(be.Ps[i], add(mul(rot_diff, mk(X.pose[i * 7] - X.pose[0], X.pose[i * 7 + 1] - X.pose[1], X.pose[i * 7 + 2] - X.pose[2])), origin_P0));
        st3(be.Vs[i], mul(rot_diff, mk(X.sb[i * 9], X.sb[i * 9 + 1], X.sb[i * 9 + 2])));
        for (int k = 0; k < 3; k++) { be.Bas[i][k] = X.sb[i * 9 + 3 + k]; be.Bgs[i][k] = X.sb[i * 9 + 6 + k]; }
        // updateLatestStates (estimator.cpp:1768-1776): latest_Bg feeds predictMotion of the next frame, whose front-end may
        // start as soon as this kernel is done (overlapping the marginalisation)
        // (the frame that completes the DYNAMIC initialisation returns without updateLatestStates, estimator.cpp:241-252)
        if (i == W && !be.init_frame) for (int k = 0; k < 3; k++) be.latest_Bg[k] = X.sb[i * 9 + 6 + k];
    }
    if (t == W + 1) {
        be.tic[0] = X.ex[0]; be.tic[1] = X.ex[1]; be.tic[2] = X.ex[2];
        stm(be.ric, q2R(qnormalized(mkq(X.ex[6], X.ex[3], X.ex[4], X.ex[5]))));
        if (cfg.estimate_td) be.td = X.td;
    }
    __syncthreads();
    if (t == 0 && be.relo_info) {
        // "relative info between two loop frame" (estimator.cpp:1034-1056): the relocalisation pose through the same gauge fix, the drift
        // between this odometry frame and the old keyframe's world (yaw + translation), the relative pose the pose graph stores
        const m3 rot_diff = ldm(sdx);
        const v3 origin_P0 = mk(sdx[9], sdx[10], sdx[11]);
        const m3 relo_r = mul(rot_diff, q2R(qnormalized(mkq(X.relo[6], X.relo[3], X.relo[4], X.relo[5]))));
        const v3 relo_t = add(mul(rot_diff, mk(X.relo[0] - X.pose[0], X.relo[1] - X.pose[1], X.relo[2] - X.pose[2])), origin_P0);
        const m3 prev_r = ldm(be.prev_relo_r);
        const double drift_yaw = R2ypr(prev_r).x - R2ypr(relo_r).x;
        const m3 dr = ypr2R(mk(drift_yaw, 0, 0));
        stm(be.drift_correct_r, dr);
        st3(be.drift_correct_t, sub(ld3(be.prev_relo_t), mul(dr, relo_t)));
        const int li = be.relo_local;
        const m3 Rl = ldm(be.Rs[li]);
        st3(be.relo_relative_t, mul(tr(relo_r), sub(ld3(be.Ps[li]), relo_t)));
        const quat qrel = R2q(mul(tr(relo_r), Rl));
        be.relo_relative_q[0] = qrel.w; be.relo_relative_q[1] = qrel.x; be.relo_relative_q[2] = qrel.y; be.relo_relative_q[3] = qrel.z;
        const double a = R2ypr(Rl).x - R2ypr(relo_r).x;   // Utility::normalizeAngle (utility.h:131-139), degrees
        be.relo_relative_yaw = a > 0 ? a - 360.0 * floor((a + 180.0) / 360.0) : a + 360.0 * floor((-a + 180.0) / 360.0);
        for (int k = 0; k < 7; k++) be.relo_Pose[k] = X.relo[k];
        be.relo_info = 0;
    }
    }   // IMU mode
    // setDepth (feature_manager.cpp:197-223)
    for (int k = t; k < nlm; k += nt) {
        int slot = c.lm_order[k];
        int pi = c.lm_pidx[slot];
        if (pi < 0) continue;
        double d = 1.0 / c.feat[pi];
        c.lm_depth[slot] = d;
        c.lm_solve[slot] = d < 0 ? 2 : 1;
    }
    __syncthreads();
    // failureDetection + clearState() / setParameter() (estimator.cpp:345-353, 1113-1159, 43-116, 15-41).  The reference runs it
    // after optimization() (solve + marginalisation) and throws the whole state away when it fires, so nothing the marginalisation
    // produces survives a reboot: it is decided HERE, before the host records ev_solve, because the reset rewrites imu_head / td /
    // ric / latest_Bg, which the next frame's front-end (fe_begin) and the IMU scatter kernel read as soon as this kernel is done.
    if (be.solver_flag == 1 && !be.init_frame) {
        if (t == 0) {
            int fail = 0;
            if (nrm(ld3(be.Bas[W])) > 2.5) fail = 1;
            if (nrm(ld3(be.Bgs[W])) > 1.0) fail = 1;
            v3 tmpP = ld3(be.Ps[W]);
            if (nrm(sub(tmpP, ld3(be.last_P))) > 5) fail = 1;
            if (fabs(tmpP.z - be.last_P[2]) > 1) fail = 1;
            sh_i[0] = fail;
        }
        __syncthreads();
        if (sh_i[0]) {
            for (int k = t; k < c.NL; k += nt) c.lm_free[k] = c.NL - 1 - k;
            if (t == 0) {
                for (int i = 0; i <= W + 1; i++) c.pre[i].valid = 0;
                for (int i = 0; i <= W; i++) {
                    for (int k = 0; k < 3; k++) { be.Ps[i][k] = 0; be.Vs[i][k] = 0; be.Bas[i][k] = 0; be.Bgs[i][k] = 0; }
                    stm(be.Rs[i], eye());
                    be.Headers[i] = 0;
                    be.pre_idx[i] = i;
                }
                // setParameter() restores the sequence's calibration (Batch::cal).  (estimate_extrinsic = 2: RIC[0], the calibrated rotation,
                // and TIC[0] = 0 -- the table's tic on such a handle)
                const vio_calibration &K = *c.K;
                for (int k = 0; k < 9; k++) be.ric[k] = cfg.estimate_extrinsic == 2 ? be.ex_ric[k] : K.ric[k];
                for (int k = 0; k < 3; k++) { be.tic[k] = K.tic[k]; be.latest_Bg[k] = 0; }
                be.td = K.td;
                be.g[0] = 0; be.g[1] = 0; be.g[2] = K.g_norm;   // setParameter(): g = G (estimator.cpp:26)
                be.first_imu = 0; be.frame_count = 0; be.solver_flag = 0; be.openExEstimation = 0; be.has_prior = 0;
                be.initFirstPoseFlag = 0; be.prevTime = -1; be.n_lm = 0; be.n_free = c.NL; be.ring_base = 0;
                be.imu_head = be.imu_count_ingest;  // clearState() empties imu_buf (samples pushed for the next frame while this one was
                                                     // being optimised - tracker lag 1 - arrived after the reset)
                be.relo_info = 0;   // relocalization_info = false (estimator.cpp:96)
                be.reboot_count++;
                be.status_code = VIO_REBOOTED;
                be.rebooted = 1;
                be.do_marg = 0;
                be.overflow = 0;
            }
        }
    }
}

}  // namespace
