// estimate_extrinsic = 2: InitialEXRotation (vins_estimator/src/initial/initial_ex_rotation.cpp) on the device.
//   ex_relative_r   solveRelativeR (:70-147): cv::findFundamentalMat(ll, rr) with its default arguments (FM_RANSAC, 3.0, 0.99) as SURVEY.md B.3
//                   builds it (7-point RANSAC with the fixed-seed sampler of fe_ransac.h, then the Hartley-normalised 8-point solution on the
//                   inliers), decomposeE and the four cv::triangulatePoints votes.
//   ex_average      CalibrationExRotation (:12-68): Huber-weighted rotation averaging over the stored (Rc, Rimu, Rc_g) pairs.
//   ex_calibrate    the per-frame phase of be_ingest<true> (estimator.cpp:208-226).
// Included by be_ingest.hip and be_stage.hip; uses block_sum, block_scan_flags, jacobi_small (be_linalg.h) and Ctx / obs_ptr (be_ctx.h).
#pragma once
#include "be_ctx.h"
#include "be_linalg.h"
#include "fe_ransac.h"

namespace {

struct ExShared {
    RansacShared R;
    double N9[81], V9[81];     // 8-point normal matrix / its eigenvectors
    double F[9];               // the fundamental matrix
    double Rc[2][9], t[3];     // R1, R2, t of decomposeE
    double A4[16], V4[16];     // A^T A of the averaging step / its eigenvectors
    double Rout[9];
    int cnt[4];                // triangulation votes of (R1, t) (R1, -t) (R2, t) (R2, -t)
    int ok;
    int win, flip;             // which of R1 / R2 was returned (1 / 2), whether decomposeE changed the sign of E (vio_stage_relative_r_detail)
};

__device__ __forceinline__ double wave_sum_d(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// eigenvalues (diagonal of A after jacobi_small) in descending order: idx[0..n)
__device__ __forceinline__ void ex_sort_desc(const double *A, int n, int *idx) {
    for (int i = 0; i < n; i++) idx[i] = i;
    for (int i = 1; i < n; i++)
        for (int j = i; j > 0 && A[idx[j] * n + idx[j]] > A[idx[j - 1] * n + idx[j - 1]]; j--) { int q = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = q; }
}
// column k of the n x n eigenvector matrix V with the sign that makes its largest-magnitude component positive (first one on a tie): the
// sign convention of every SVD / eigenvector below (the restatement in tests/excalib_ref.py uses the same one)
__device__ __forceinline__ void ex_canon_col(const double *V, int n, int k, double *out) {
    int im = 0;
    for (int i = 1; i < n; i++) if (fabs(V[i * n + k]) > fabs(V[im * n + k])) im = i;
    const double sg = V[im * n + k] < 0 ? -1.0 : 1.0;
    for (int i = 0; i < n; i++) out[i] = sg * V[i * n + k];
}

// solveRelativeR for n correspondences (x1, y1) of frame l -> (x2, y2) of frame r, already rounded to float32 (cv::Point2f), held in LDS.
// All threads of the (256-thread) workgroup call it; S.Rout receives the result (row-major), valid after the call.
__device__ void ex_relative_r(int n, const double *X1, const double *Y1, const double *X2, const double *Y2, int *status, ExShared &S) {
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63;
    if (t == 0) { for (int k = 0; k < 9; k++) S.Rout[k] = (k % 4 == 0) ? 1.0 : 0.0; S.ok = 0; }
    __syncthreads();
    if (n < 9) return;   // Identity for fewer than 9 correspondences (:72, :146)
    // ---- cv::findFundamentalMat(ll, rr): RANSAC, threshold 3.0 (normalised units: every point of a sane model is an inlier), 1000 iterations
    ransac_block(9.0, 1000, n, X1, Y1, X2, Y2, status, S.R, nullptr);
    // ---- run8Point on the inliers (one wavefront)
    if (t < 64 && S.R.maxGood > 0) {
        double c1x = 0, c1y = 0, c2x = 0, c2y = 0, cn = 0;
        for (int i = lane; i < n; i += 64)
            if (status[i]) { c1x += X1[i]; c1y += Y1[i]; c2x += X2[i]; c2y += Y2[i]; cn += 1.0; }
        c1x = wave_sum_d(c1x); c1y = wave_sum_d(c1y); c2x = wave_sum_d(c2x); c2y = wave_sum_d(c2y); cn = wave_sum_d(cn);
        const double inv = 1.0 / cn;
        c1x *= inv; c1y *= inv; c2x *= inv; c2y *= inv;
        double sc1 = 0, sc2 = 0;
        for (int i = lane; i < n; i += 64)
            if (status[i]) {
                sc1 += sqrt((X1[i] - c1x) * (X1[i] - c1x) + (Y1[i] - c1y) * (Y1[i] - c1y));
                sc2 += sqrt((X2[i] - c2x) * (X2[i] - c2x) + (Y2[i] - c2y) * (Y2[i] - c2y));
            }
        sc1 = wave_sum_d(sc1) * inv; sc2 = wave_sum_d(sc2) * inv;
        const bool good = cn >= 8 && sc1 >= 1.1920928955078125e-07 && sc2 >= 1.1920928955078125e-07;
        if (good) {
            sc1 = sqrt(2.0) / sc1; sc2 = sqrt(2.0) / sc2;
            // the 9 x 9 normal matrix sum r r^T, r = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1), one entry per reduction
            for (int e = 0; e < 45; e++) {
                int a = 0, rem = e;
                while (rem >= 9 - a) { rem -= 9 - a; a++; }
                const int b = a + rem;
                double acc = 0;
                for (int i = lane; i < n; i += 64) {
                    if (!status[i]) continue;
                    const double x1 = (X1[i] - c1x) * sc1, y1 = (Y1[i] - c1y) * sc1, x2 = (X2[i] - c2x) * sc2, y2 = (Y2[i] - c2y) * sc2;
                    const double r[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
                    double ra = r[0], rb = r[0];
#pragma unroll
                    for (int q = 1; q < 9; q++) { if (q == a) ra = r[q]; if (q == b) rb = r[q]; }
                    acc += ra * rb;
                }
                acc = wave_sum_d(acc);
                if (lane == 0) { S.N9[a * 9 + b] = acc; S.N9[b * 9 + a] = acc; }
            }
        }
        if (lane == 0) {
            int ok = 0;
            if (good) {
                jacobi_small(S.N9, S.V9, 9);
                int idx[9];
                ex_sort_desc(S.N9, 9, idx);
                int i = 0;
                for (; i < 9; i++) if (fabs(S.N9[idx[i] * 10]) < 2.220446049250313e-16) break;
                if (i >= 8) {
                    double f[9], F0[9];
                    ex_canon_col(S.V9, 9, idx[8], f);
                    for (int k = 0; k < 9; k++) F0[k] = f[k];
                    // rank 2: drop the smallest singular direction v3 of F0 (F0 <- F0 - (F0 v3) v3^T = U diag(w0, w1, 0) V^T)
                    double G[9], Vg[9];
                    for (int p = 0; p < 3; p++) for (int q = 0; q < 3; q++) G[p * 3 + q] = F0[p] * F0[q] + F0[3 + p] * F0[3 + q] + F0[6 + p] * F0[6 + q];
                    jacobi_small(G, Vg, 3);
                    int ig[3];
                    ex_sort_desc(G, 3, ig);
                    double v3[3];
                    ex_canon_col(Vg, 3, ig[2], v3);
                    for (int p = 0; p < 3; p++) {
                        const double fv = F0[p * 3] * v3[0] + F0[p * 3 + 1] * v3[1] + F0[p * 3 + 2] * v3[2];
                        for (int q = 0; q < 3; q++) F0[p * 3 + q] -= fv * v3[q];
                    }
                    // F = T2^T F0 T1, then F(2,2) = 1
                    const double T1[9] = {sc1, 0, -sc1 * c1x, 0, sc1, -sc1 * c1y, 0, 0, 1}, T2[9] = {sc2, 0, -sc2 * c2x, 0, sc2, -sc2 * c2y, 0, 0, 1};
                    double M[9], Fm[9];
                    for (int p = 0; p < 3; p++) for (int q = 0; q < 3; q++) M[p * 3 + q] = F0[p * 3] * T1[q] + F0[p * 3 + 1] * T1[3 + q] + F0[p * 3 + 2] * T1[6 + q];
                    for (int p = 0; p < 3; p++) for (int q = 0; q < 3; q++) Fm[p * 3 + q] = T2[p] * M[q] + T2[3 + p] * M[3 + q] + T2[6 + p] * M[6 + q];
                    if (fabs(Fm[8]) > 1.1920928955078125e-07) { const double s8 = 1.0 / Fm[8]; for (int k = 0; k < 9; k++) Fm[k] *= s8; }
                    for (int k = 0; k < 9; k++) S.F[k] = Fm[k];
                    // ---- decomposeE (:149-160): E = U diag V^T.  An essential matrix has two equal singular values, so only the null vector v3
                    // of E (smallest eigenvector of E^T E, canonical sign) and the orientation of the other two are defined: v1 = the largest
                    // eigenvector, v2 = v3 x v1 (U W V^T does not change under a rotation of (v1, v2) in their plane, a reflection swaps R1 and R2);
                    // u_k = E v_k / |E v_k| (k < 2), u3 = u1 x u2; R1 = U W V^T, R2 = U W^T V^T, t = u3.  det(R1) = -1: E = -E, i.e. R1, R2 and
                    // t change sign (:128-132)
                    for (int p = 0; p < 3; p++) for (int q = 0; q < 3; q++) G[p * 3 + q] = Fm[p] * Fm[q] + Fm[3 + p] * Fm[3 + q] + Fm[6 + p] * Fm[6 + q];
                    jacobi_small(G, Vg, 3);
                    ex_sort_desc(G, 3, ig);
                    double V[3][3], U[3][3];
                    ex_canon_col(Vg, 3, ig[0], V[0]);
                    ex_canon_col(Vg, 3, ig[2], V[2]);
                    V[1][0] = V[2][1] * V[0][2] - V[2][2] * V[0][1];
                    V[1][1] = V[2][2] * V[0][0] - V[2][0] * V[0][2];
                    V[1][2] = V[2][0] * V[0][1] - V[2][1] * V[0][0];
                    for (int k = 0; k < 2; k++) {
                        double u[3], nu = 0;
                        for (int p = 0; p < 3; p++) { u[p] = Fm[p * 3] * V[k][0] + Fm[p * 3 + 1] * V[k][1] + Fm[p * 3 + 2] * V[k][2]; nu += u[p] * u[p]; }
                        nu = nu > 0 ? 1.0 / sqrt(nu) : 0.0;
                        for (int p = 0; p < 3; p++) U[k][p] = u[p] * nu;
                    }
                    U[2][0] = U[0][1] * U[1][2] - U[0][2] * U[1][1];
                    U[2][1] = U[0][2] * U[1][0] - U[0][0] * U[1][2];
                    U[2][2] = U[0][0] * U[1][1] - U[0][1] * U[1][0];
                    // U W V^T = -u1 v2^T + u2 v1^T + u3 v3^T,  U W^T V^T = u1 v2^T - u2 v1^T + u3 v3^T
                    for (int p = 0; p < 3; p++)
                        for (int q = 0; q < 3; q++) {
                            const double a12 = U[0][p] * V[1][q], a21 = U[1][p] * V[0][q], a33 = U[2][p] * V[2][q];
                            S.Rc[0][p * 3 + q] = (a21 - a12) + a33;
                            S.Rc[1][p * 3 + q] = (a12 - a21) + a33;
                        }
                    for (int p = 0; p < 3; p++) S.t[p] = U[2][p];
                    const double *R1 = S.Rc[0];
                    const double d1 = R1[0] * (R1[4] * R1[8] - R1[5] * R1[7]) - R1[1] * (R1[3] * R1[8] - R1[5] * R1[6]) + R1[2] * (R1[3] * R1[7] - R1[4] * R1[6]);
                    S.flip = d1 + 1.0 < 1e-09;
                    if (S.flip) {
                        for (int k = 0; k < 9; k++) { S.Rc[0][k] = -S.Rc[0][k]; S.Rc[1][k] = -S.Rc[1][k]; }
                        for (int p = 0; p < 3; p++) S.t[p] = -S.t[p];
                    }
                    ok = 1;
                }
            }
            S.ok = ok;
            for (int k = 0; k < 4; k++) S.cnt[k] = 0;
        }
    }
    __syncthreads();
    if (!S.ok) return;   // no model (the reference's findFundamentalMat returns an empty matrix): the pair is taken as the identity
    // ---- testTriangulation (:100-125) of (R1, t) (R1, -t) (R2, t) (R2, -t) over ALL correspondences: cv::triangulatePoints with P = [I | 0] and
    // P1 = [R | t] in float (Matx34f), DLT by the smallest eigenvector of the 4 x 4 A^T A, a point counts when it lies in front of both cameras
    for (int it = t; it < 4 * n; it += nt) {
        const int h = it / n, i = it - h * n;
        const double sg = (h & 1) ? -1.0 : 1.0;
        const double *Rh = S.Rc[h >> 1];
        double P1[12];
        for (int p = 0; p < 3; p++) {
            for (int q = 0; q < 3; q++) P1[p * 4 + q] = (double)(float)Rh[p * 3 + q];
            P1[p * 4 + 3] = (double)(float)(sg * S.t[p]);
        }
        const double x1 = X1[i], y1 = Y1[i], x2 = X2[i], y2 = Y2[i];
        double A[16];
        for (int k = 0; k < 4; k++) {
            const double P2k = k == 2 ? 1.0 : 0.0, P0k = k == 0 ? 1.0 : 0.0, P1k = k == 1 ? 1.0 : 0.0;
            A[k] = x1 * P2k - P0k;
            A[4 + k] = y1 * P2k - P1k;
            A[8 + k] = x2 * P1[8 + k] - P1[k];
            A[12 + k] = y2 * P1[8 + k] - P1[4 + k];
        }
        double N[16], Vn[16];
        for (int p = 0; p < 4; p++) for (int q = 0; q < 4; q++) N[p * 4 + q] = A[p] * A[q] + A[4 + p] * A[4 + q] + A[8 + p] * A[8 + q] + A[12 + p] * A[12 + q];
        jacobi_small(N, Vn, 4);
        int mi = 0;
        for (int q = 1; q < 4; q++) if (N[q * 5] < N[mi * 5]) mi = q;
        const double X = Vn[mi], Y = Vn[4 + mi], Z = Vn[8 + mi], Wh = Vn[12 + mi];
        const double zl = Z / Wh, zr = (P1[8] * X + P1[9] * Y + P1[10] * Z + P1[11] * Wh) / Wh;
        if (zl > 0 && zr > 0) atomicAdd(&S.cnt[h], 1);
    }
    __syncthreads();
    if (t == 0) {
        const int r1 = max(S.cnt[0], S.cnt[1]), r2 = max(S.cnt[2], S.cnt[3]);
        const double *ans = S.Rc[r1 > r2 ? 0 : 1];   // ratio1 > ratio2 ? R1 : R2 (a tie takes R2)
        S.win = r1 > r2 ? 1 : 2;
        for (int p = 0; p < 3; p++) for (int q = 0; q < 3; q++) S.Rout[q * 3 + p] = ans[p * 3 + q];   // ans_R_eigen(j, i) = ans_R_cv(i, j)
    }
    __syncthreads();
}

// L(q) - R(p) of CalibrationExRotation (:36-50) for q = q(Rc), p = q(Rimu), w x y z each; row-major 4 x 4, quaternion vector part first
__device__ __forceinline__ void ex_LmR(const double *q, const double *p, double *M) {
    const double dw = q[0] - p[0];
    const double sx = q[1] + p[1], sy = q[2] + p[2], sz = q[3] + p[3];   // skew(qv) + skew(pv)
    M[0] = dw;  M[1] = -sz; M[2] = sy;  M[3] = q[1] - p[1];
    M[4] = sz;  M[5] = dw;  M[6] = -sx; M[7] = q[2] - p[2];
    M[8] = -sy; M[9] = sx;  M[10] = dw; M[11] = q[3] - p[3];
    M[12] = -(q[1] - p[1]); M[13] = -(q[2] - p[2]); M[14] = -(q[3] - p[3]); M[15] = dw;
}

// the averaging step over the stored pairs: A^T A (4 x 4, FP64) of the stacked blocks huber (L - R), Jacobi eigen-solve, sigma = sqrt(lambda);
// the new ric and the singular values go to X.  Returns (on thread 0) whether the calibration succeeded.
__device__ bool ex_average(ExSeq &X, const double *hist, int W, ExShared &S, double *sred) {
    const int t = threadIdx.x, nt = blockDim.x;
    double acc[10];
    for (int k = 0; k < 10; k++) acc[k] = 0;
    for (int i = t; i < X.count; i += nt) {
        const double *pr = hist + (size_t)((X.head + i) % VIO_EXCALIB_CAP) * VIO_EXCALIB_PAIR_D;
        const double *qc = pr, *qi = pr + 4, *qg = pr + 8;
        // angularDistance(Rc, Rc_g) = 2 atan2(|(qc qg^*).vec|, |(qc qg^*).w|)
        const double dw = qc[0] * qg[0] + qc[1] * qg[1] + qc[2] * qg[2] + qc[3] * qg[3];
        const double dx = -qc[0] * qg[1] + qc[1] * qg[0] - qc[2] * qg[3] + qc[3] * qg[2];
        const double dy = -qc[0] * qg[2] + qc[2] * qg[0] - qc[3] * qg[1] + qc[1] * qg[3];
        const double dz = -qc[0] * qg[3] + qc[3] * qg[0] - qc[1] * qg[2] + qc[2] * qg[1];
        const double ang = 180.0 / M_PI * (2.0 * atan2(sqrt(dx * dx + dy * dy + dz * dz), fabs(dw)));
        const double hub = ang > 5.0 ? 5.0 / ang : 1.0;
        double M[16];
        ex_LmR(qc, qi, M);
        int e = 0;
        for (int a = 0; a < 4; a++)
            for (int b = a; b < 4; b++, e++) acc[e] += hub * hub * (M[a] * M[b] + M[4 + a] * M[4 + b] + M[8 + a] * M[8 + b] + M[12 + a] * M[12 + b]);
    }
    for (int e = 0; e < 10; e++) acc[e] = block_sum(acc[e], sred);
    bool ok = false;
    if (t == 0) {
        int e = 0;
        for (int a = 0; a < 4; a++) for (int b = a; b < 4; b++, e++) { S.A4[a * 4 + b] = acc[e]; S.A4[b * 4 + a] = acc[e]; }
        jacobi_small(S.A4, S.V4, 4);
        int idx[4];
        ex_sort_desc(S.A4, 4, idx);
        for (int k = 0; k < 4; k++) X.sv[k] = sqrt(fmax(S.A4[idx[k] * 5], 0.0));
        double x[4];
        ex_canon_col(S.V4, 4, idx[3], x);
        // Quaterniond estimated_R(x): coefficients in (x, y, z, w) order; ric = estimated_R.toRotationMatrix().inverse()
        const m3 Rq = q2R(mkq(x[3], x[0], x[1], x[2]));
        stm(X.ric, tr(Rq));
        ok = X.calls >= W && X.sv[2] > 0.25;
    }
    return ok;
}

// The per-frame phase of be_ingest<true> (estimator.cpp:208-226) for a calibrating sequence with frame_count != 0: correspondences of
// window frames fc - 1 and fc in landmark-list order (FeatureManager::getCorresponding) into LDS (pts: >= 4 * NP doubles), solveRelativeR,
// append (Rc, Rimu = delta_q of slot fc, Rc_g = ric^-1 Rimu ric) to the history, average.  On success the sequence's ric becomes the estimate
// (ric[0] = RIC[0] = calib_ric, ESTIMATE_EXTRINSIC = 1).  All threads call it.
__device__ void ex_calibrate(const Batch &B, Ctx &c, int s, int fc, int nlm, double *pts, int *scratch, double *sred, ExShared &S) {
    const int t = threadIdx.x, nt = blockDim.x, NP = B.gNP;
    BeSeq &be = *c.be;
    const DevCfg &C = *B.cfg;
    ExSeq &X = C.exc[s];
    double *hist = C.exh + (size_t)s * VIO_EXCALIB_CAP * VIO_EXCALIB_PAIR_D;
    int *flag = c.lm_tmp, *offs = c.lm_pidx;   // (temporaries of addFeatureCheckParallax, free again)
    for (int k = t; k < nlm; k += nt) {
        const int slot = c.lm_order[k], st = c.lm_start[slot];
        flag[k] = (st <= fc - 1 && st + c.lm_nobs[slot] - 1 >= fc) ? 1 : 0;
    }
    __syncthreads();
    const int ntot = block_scan_flags(flag, nlm, offs, scratch);
    const int n = min(ntot, NP);
    double *X1 = pts, *Y1 = X1 + NP, *X2 = Y1 + NP, *Y2 = X2 + NP;
    for (int k = t; k < nlm; k += nt) {
        if (!flag[k] || offs[k] >= n) continue;
        const int slot = c.lm_order[k], j = offs[k];
        const double *a = obs_ptr(c, slot, fc - 1), *b = obs_ptr(c, slot, fc);
        X1[j] = (double)(float)a[0]; Y1[j] = (double)(float)a[1];
        X2[j] = (double)(float)b[0]; Y2[j] = (double)(float)b[1];
    }
    __syncthreads();
    ex_relative_r(n, X1, Y1, X2, Y2, flag, S);
    if (t == 0) {
        const PreInt &P = c.pre[be.pre_idx[fc]];
        const m3 Rc = ldm(S.Rout), Rimu = q2R(mkq(P.dq[0], P.dq[1], P.dq[2], P.dq[3])), ric = ldm(X.ric);
        const m3 Rcg = mul(mul(tr(ric), Rimu), ric);
        int slot;
        if (X.count == VIO_EXCALIB_CAP) { slot = X.head; X.head = (X.head + 1) % VIO_EXCALIB_CAP; be.overflow |= 128; }
        else { slot = (X.head + X.count) % VIO_EXCALIB_CAP; X.count++; }
        double *pr = hist + (size_t)slot * VIO_EXCALIB_PAIR_D;
        const quat q0 = R2q(Rc), q1 = R2q(Rimu), q2 = R2q(Rcg);
        const quat qs[3] = {q0, q1, q2};
        for (int k = 0; k < 3; k++) { pr[4 * k] = qs[k].w; pr[4 * k + 1] = qs[k].x; pr[4 * k + 2] = qs[k].y; pr[4 * k + 3] = qs[k].z; }
        X.calls++;
    }
    __syncthreads();
    const bool ok = ex_average(X, hist, c.W, S, sred);
    if (t == 0 && ok) {
        for (int k = 0; k < 9; k++) { be.ric[k] = X.ric[k]; be.ex_ric[k] = X.ric[k]; }
        be.ex_pending = 0;
        X.success_frame = be.frames_processed + 1;   // the count after this frame (the tail of be_ingest adds it)
    }
    __syncthreads();
}

}  // namespace
