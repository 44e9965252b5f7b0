// RANSAC pieces of cv::findFundamentalMat shared by the front-end (rejectWithF, fe_kernels.hip) and the
// extrinsic-rotation calibration of be_ingest (InitialEXRotation::solveRelativeR, be_excalib.h).
#pragma once
#include <hip/hip_runtime.h>
#include "vio_state.h"

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double det3(const double *F) {
    return F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
}
__device__ int solve_cubic_det(double c3, double c2, double c1, double c0, double roots[3]) {
    double mx = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
    if (mx == 0.0) return 0;
    if (fabs(c3) < 1e-12 * mx) {
        if (fabs(c2) < 1e-12 * mx) {
            if (fabs(c1) < 1e-12 * mx) return 0;
            roots[0] = -c0 / c1;
            return 1;
        }
        double disc = c1 * c1 - 4 * c2 * c0;
        if (disc < 0) return 0;
        double sq = sqrt(disc);
        roots[0] = (-c1 + sq) / (2 * c2);
        roots[1] = (-c1 - sq) / (2 * c2);
        return 2;
    }
    double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    double Bd = 1.0 + fmax(fabs(a), fmax(fabs(b), fabs(c)));
    double lo = -Bd, hi = Bd;
    for (int i = 0; i < 100; i++) {
        double mid = 0.5 * (lo + hi);
        double f = ((mid + a) * mid + b) * mid + c;
        if (f > 0) hi = mid; else lo = mid;
    }
    double r = 0.5 * (lo + hi);
    for (int i = 0; i < 2; i++) {
        double f = ((r + a) * r + b) * r + c, fp = (3 * r + 2 * a) * r + b;
        if (fp != 0.0) r -= f / fp;
    }
    roots[0] = r;
    double p = a + r, q = b + r * p;
    double disc = p * p - 4 * q;
    if (disc < 0) return 1;
    double sq = sqrt(disc);
    roots[1] = (-p + sq) * 0.5;
    roots[2] = (-p - sq) * 0.5;
    return 3;
}
// The 7-point solver (cv::findFundamentalMat's minimal solver) for ONE minimal sample on ONE wavefront.
// Lane e = 9 r + c (e < 63) owns element (r, c) of the 7 x 9 epipolar system and goes through the Gauss-Jordan elimination with
// full pivoting element-wise: the pivot is a wave-wide arg-max (first maximum in row-major order, like the scalar scan), row and
// column exchanges are one LDS round trip, and every element performs exactly the scalar algorithm's operations on it
// (a *= inv in the pivot row, a -= f * (pivot-row element * inv) elsewhere) -- same roundings, hence the same null space bit for bit,
// in 7 short steps instead of a 120 us scalar elimination on private (scratch) arrays.
// ws: 96 doubles of LDS private to the wavefront.  Fout: 27 doubles.  Returns the number of models (uniform over the wavefront).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ int seven_point_wave(double a, double *ws, double *Fout) {
    const int lane = threadIdx.x & 63;
    const int r = lane / 9, c = lane - 9 * r;   // lane 63: r = 7, never eligible
    double *As = ws, *f1s = ws + 64, *f2s = ws + 73;
    double amax = lane < 63 ? fabs(a) : 0.0;
    for (int off = 32; off > 0; off >>= 1) amax = fmax(amax, __shfl_xor(amax, off, 64));
    const double tol = 1e-12 * amax;
    unsigned long long perm = 0x876543210ULL;   // nibble i = perm[i]
    int rank = 0;
    for (int i = 0; i < 7; i++) {
        double v = (lane < 63 && r >= i && c >= i) ? fabs(a) : -1.0;
        int idx = lane;
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(v, off, 64);
            const int oi = __shfl_xor(idx, off, 64);
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        if (!(v > tol)) break;   // rank-deficient sample: the remaining columns are free
        const int pr = idx / 9, pc = idx - 9 * pr;
        wave_lds_sync();
        As[lane] = a;
        wave_lds_sync();
        const int sr = r == i ? pr : (r == pr ? i : r);
        const int scol = c == i ? pc : (c == pc ? i : c);
        if (pc != i) {
            const unsigned long long ni = (perm >> (4 * i)) & 15ULL, np_ = (perm >> (4 * pc)) & 15ULL;
            perm = (perm & ~((15ULL << (4 * i)) | (15ULL << (4 * pc)))) | (np_ << (4 * i)) | (ni << (4 * pc));
        }
        if (lane < 63) {
            const double ap = As[sr * 9 + scol];          // my element after the two exchanges
            const double inv = 1.0 / As[pr * 9 + pc];     // the pivot
            const double prow = As[pr * 9 + scol] * inv;  // scaled pivot-row element of my column
            const double f = As[sr * 9 + pc];             // my row's entry in the pivot column
            if (r == i) a = prow;
            else if (f != 0.0) a = ap - f * prow;
            else a = ap;
        }
        rank = i + 1;
    }
    wave_lds_sync();
    As[lane] = a;
    wave_lds_sync();
    if (lane < 9) {   // f1[perm[i]] = -A[i][7], f2[perm[i]] = -A[i][8] (i < rank); f1[perm[7]] = 1, f2[perm[8]] = 1; other free columns 0
        int i = 0;
        for (int k = 0; k < 9; k++) if ((int)((perm >> (4 * k)) & 15ULL) == lane) i = k;
        double v1 = 0.0, v2 = 0.0;
        if (i < rank) { v1 = -As[i * 9 + 7]; v2 = -As[i * 9 + 8]; }
        if (i == 7) v1 = 1.0;
        if (i == 8) v2 = 1.0;
        f1s[lane] = v1; f2s[lane] = v2;
    }
    wave_lds_sync();
    double f1[9], f2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { f1[k] = f1s[k]; f2[k] = f2s[k]; }
    // det(f1 + l f2) = c0 + c1 l + c2 l^2 + c3 l^3 (every lane computes the same numbers)
    double c0 = det3(f1), c3 = det3(f2), c1 = 0, c2 = 0;
#pragma unroll
    for (int rr = 0; rr < 3; rr++) {
        double t[9];
#pragma unroll
        for (int q = 0; q < 9; q++) t[q] = (q / 3 == rr) ? f2[q] : f1[q];
        c1 += det3(t);
#pragma unroll
        for (int q = 0; q < 9; q++) t[q] = (q / 3 == rr) ? f1[q] : f2[q];
        c2 += det3(t);
    }
    double roots[3] = {0.0, 0.0, 0.0};
    const int nr = solve_cubic_det(c3, c2, c1, c0, roots);
    if (lane < 27) {
        const int k = lane / 9, q = lane - 9 * k;
        double fa = f1[0], fb = f2[0];
#pragma unroll
        for (int j = 1; j < 9; j++) if (q == j) { fa = f1[j]; fb = f2[j]; }
        const double rt = k == 0 ? roots[0] : (k == 1 ? roots[1] : roots[2]);
        if (k < nr) Fout[lane] = fa + rt * fb;
    }
    return nr;
}
__device__ __forceinline__ bool f_inlier(const double *f, double x1, double y1, double x2, double y2, double thr2) {
    double a = f[0] * x1 + f[1] * y1 + f[2], b = f[3] * x1 + f[4] * y1 + f[5], cc = f[6] * x1 + f[7] * y1 + f[8];
    double s2 = 1.0 / (a * a + b * b), d2 = x2 * a + y2 * b + cc;
    double a1 = f[0] * x2 + f[3] * y2 + f[6], b1 = f[1] * x2 + f[4] * y2 + f[7], c1 = f[2] * x2 + f[5] * y2 + f[8];
    double s1 = 1.0 / (a1 * a1 + b1 * b1), d1 = x1 * a1 + y1 * b1 + c1;
    double err = fmax(d1 * d1 * s1, d2 * d2 * s2);
    return err <= thr2;
}
__device__ int ransac_update_iters(double p, double ep, int modelPoints, int maxIters) {
    p = fmin(fmax(p, 0.), 1.);
    ep = fmin(fmax(ep, 0.), 1.);
    double num = fmax(1. - p, 2.2250738585072014e-308);
    double denom = 1. - pow(1. - ep, (double)modelPoints);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= maxIters * (-denom) ? maxIters : (int)rint(num / denom);
}

// RANSAC over normalised correspondences held in LDS; writes status flags.  All threads of the block participate (4 wavefronts).
// The iterations are the sequential algorithm's (sample `it` is a function of `it` alone, the iteration bound adapts after every
// accepted model in iteration order); they are evaluated in rounds: every wavefront solves `per` minimal samples (one in the first
// round -- with mostly inliers the bound falls below the round size at once --, up to 4 while many iterations remain), the inliers of
// all their models are counted by all threads (integer counts), thread 0 then replays the acceptance logic in iteration order.
#define RS_MAXB 16   // samples per round at most
struct RansacShared {
    double F[RS_MAXB * 27];
    double ws[4][96];
    int nm[RS_MAXB];
    int cnt[RS_MAXB * 3];
    double bestF[9];
    int niters, maxGood, base, batch;
};
// thr2: squared inlier threshold in the units of the points; max_iters: the RANSAC iteration cap.
__device__ __forceinline__ void ransac_block(double thr2, int max_iters, int N, const double *X1, const double *Y1, const double *X2, const double *Y2,
                             int *status, RansacShared &R, int *iters_out, float *tm = nullptr) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, nw = blockDim.x >> 6;
    long long rt0 = (tm && t == 0) ? VIO_CLOCK() : 0;
#define RS_PH(k) do { if (VIO_TIMERS && tm && t == 0) { long long n_ = VIO_CLOCK(); tm[k] += (float)(n_ - rt0); rt0 = n_; } } while (0)
    if (t == 0) { R.niters = max_iters; R.maxGood = 0; R.base = 0; R.batch = min(nw, 4); }
    __syncthreads();
    while (true) {
        const int base = R.base, niters = R.niters, batch = R.batch;
        if (base >= niters) break;
        for (int p = t; p < batch * 3; p += blockDim.x) R.cnt[p] = 0;
        if (wv < 4)
            for (int hh = wv; hh < batch; hh += min(nw, 4)) {
                const int it = base + hh;
                int nm = 0;
                if (it < niters) {
                    uint64_t sd = 0x5649464D41545258ULL + (uint64_t)it * 0xD1B54A32D192ED03ULL;
                    int idx[7];
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        bool dup;
                        int rr;
                        do {
                            rr = (int)(splitmix64(sd) % (uint64_t)N);
                            dup = false;
#pragma unroll
                            for (int j = 0; j < k; j++) dup |= (idx[j] == rr);
                        } while (dup);
                        idx[k] = rr;
                    }
                    const int r = lane / 9, cc = lane - 9 * r;
                    int my = idx[0];
#pragma unroll
                    for (int k = 1; k < 7; k++) if (r == k) my = idx[k];
                    const double x1 = X1[my], y1 = Y1[my], x2 = X2[my], y2 = Y2[my];
                    // A[i] = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1)
                    const double u = cc < 3 ? x2 : (cc < 6 ? y2 : 1.0);
                    const int c3 = cc - 3 * (cc / 3);
                    const double w_ = c3 == 0 ? x1 : (c3 == 1 ? y1 : 1.0);
                    const double a = cc < 6 ? (c3 == 2 ? u : u * w_) : w_;
                    nm = seven_point_wave(a, R.ws[wv], &R.F[hh * 27]);
                }
                if (lane == 0) R.nm[hh] = nm;
            }
        __syncthreads();
        RS_PH(0);
        for (int i0 = 0; i0 < N; i0 += blockDim.x) {
            const int i = i0 + t;
            const bool have = i < N;
            const double x1 = have ? X1[i] : 0.0, y1 = have ? Y1[i] : 0.0, x2 = have ? X2[i] : 0.0, y2 = have ? Y2[i] : 0.0;
            for (int hh = 0; hh < batch; hh++) {
                const int nm = R.nm[hh];
                for (int m = 0; m < nm; m++) {
                    const bool good = have && f_inlier(&R.F[hh * 27 + m * 9], x1, y1, x2, y2, thr2);
                    const unsigned long long bal = __ballot(good);
                    if (lane == 0 && bal) atomicAdd(&R.cnt[hh * 3 + m], __popcll(bal));
                }
            }
        }
        __syncthreads();
        RS_PH(1);
        if (t == 0) {
            int ni = R.niters, mg = R.maxGood;
            for (int hh = 0; hh < batch; hh++) {
                int it = base + hh;
                if (it >= ni) break;
                for (int m = 0; m < R.nm[hh]; m++) {
                    int good = R.cnt[hh * 3 + m];
                    if (good > max(mg, 6)) {
                        mg = good;
                        for (int q = 0; q < 9; q++) R.bestF[q] = R.F[hh * 27 + m * 9 + q];
                        ni = ransac_update_iters(0.99, (double)(N - good) / N, 7, ni);
                    }
                }
            }
            R.niters = ni;
            R.maxGood = mg;
            R.base = base + batch;
            const int left = ni - (base + batch);
            R.batch = left >= 4 * RS_MAXB ? RS_MAXB : (left > 8 ? 8 : 4);
        }
        __syncthreads();
        RS_PH(2);
    }
    int mg = R.maxGood;
    for (int i = t; i < N; i += blockDim.x) status[i] = (mg > 0 && f_inlier(R.bestF, X1[i], Y1[i], X2[i], Y2[i], thr2)) ? 1 : 0;
    if (t == 0 && iters_out) *iters_out = R.niters;
    __syncthreads();
    RS_PH(3);
#undef RS_PH
}

}  // namespace
