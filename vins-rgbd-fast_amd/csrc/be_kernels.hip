// Back-end kernels (gfx950, FP64): Estimator::processImage (vins_estimator/src/estimator/estimator.cpp:156-374) batched
// over S sequences, one workgroup per sequence, three launches per frame (be_finish runs inside the be_marg kernel); the block
// primitives and dense linear algebra live in be_linalg.h:
//   be_ingest  addFeatureCheckParallax (feature_manager.cpp:56-123), getIMUInterval/processIMU (estimator.cpp:118-154,
//              1910-1942, IntegrationBase::propagate), triangulateWithDepth (feature_manager.cpp:386-543)
//   be_solve   optimization() (estimator.cpp:1161-1368): the Ceres DENSE_SCHUR + traditional-DOGLEG solve replaced by a
//              bespoke trust-region (dogleg / LM-regularised Gauss-Newton) solver: batched residual/Jacobian evaluation,
//              frame-pair blocked J^T J, landmark Schur complement, dense Cholesky, step control as SURVEY.md App. B.5
//   be_marg    marginalisation (estimator.cpp:1370-1575, marginalization_factor.cpp:181-315) in the canonical layout
//   be_finish  movingConsistencyCheck, failureDetection, slideWindow, removeFailures, odometry row
// This unit: be_solve (the phased solver, be_phased.h, and the persistent one below), be_marg and be_finish; be_ingest is be_ingest.hip.  What
// they share is in be_ctx.h, be_preint.h and be_solve_common.h.  The solvers and the marginalisation stay one unit because apart they compile
// to other code than together, and so do the factor stage kernels at the end.
#include "be_solve_common.h"
#include "be_phased.h"

// ====================================================================================================== be_solve
namespace {

// evaluate every residual at X. withJ: store weighted Jacobians/residuals for assembly. Returns total cost.
// vext: the extrinsic and / or td block is a variable of this solve.  Otherwise the residual records are written in the compact
// layout (28 doubles: two rows of [pose_i(6) pose_j(6) inv_depth r]) and no Jacobian is evaluated for the constant blocks.
__device__ __forceinline__ double evaluate(const Ctx &c, const Params &X, const double *feat, bool withJ, int nres, double *sred, double *sdx, double *srp,
                                           double *geo, bool vext) {
    const int t = threadIdx.x, nt = blockDim.x, W = c.W, n = c.NPR;
    const BeSeq &be = *c.be;
    const vio_config &cfg = c.C->c;
    double cost = 0;
    const int s = c.s;
    struct { float *timings; } B = {c.timings};
    PH_INIT;
    // Stage 1 (independent small jobs, one barrier for all of them): prior tangent dx (threads 0 .. W + 2), IMU factors (upper
    // wavefronts), frame-pair geometry (threads 0 .. W1^2).  Stage 2: prior mat-vec, then the projection residuals.
    if (be.has_prior) prior_dx(c, X, sdx, false);
    PH(40);
    // IMU factors: five threads per factor (whitened residual + four Jacobian column groups). Spread over the upper lanes
    // of the block so that they do not serialise with the projection residuals handled by the low thread ids.
    v3 G = ld3(be.g);
    auto imu_item = [&](int i, int part) {
        const int j = i + 1;
        const PreInt &p = c.pre[be.pre_idx[j]];
        bf::imu_work_item(p, !cfg.use_imu || bf::imu_solver_skips(p), G, &X.pose[i * 7], &X.sb[i * 9], &X.pose[j * 7], &X.sb[j * 9], part, withJ,
                          c.imu_raw + (size_t)i * 15 * 31, cost);
    };
    {
        // Five work types per factor (whitened residual + four Jacobian column groups), each a different code path.  With at least
        // five wavefronts every type gets its own wavefront (the top five, factor i on lane 63 - i), so that the types run side by
        // side instead of one wavefront executing its divergent branches one after the other; the upper lanes are used because the
        // low thread ids carry the first projection residuals.
        const int nwv = nt >> 6, part = nwv - 1 - (t >> 6), i = 63 - (t & 63);
        if (nwv >= 5 && W <= 64) {
            if (part < 5 && i < W) imu_item(i, part);
        } else {
            for (int w = (nt - 1 - t); w < W * 5; w += nt) imu_item(w / 5, w % 5);
        }
    }
    PH(46);
    // projection factors, CauchyLoss(1.0): frame-pair geometry first (one thread per pair with residuals), then one thread per
    // residual with a handful of 3-vector products (be_factors.h eval_projection_pair).  The pair geometry lives in LDS (`geo`,
    // (W1^2 + 1) x 32 doubles of the work region, free whenever evaluate runs): every residual gathers 30 doubles of it, and as
    // per-lane gathers from HBM those were a third of the cache-line lookups that bound this loop.
    {
        const int W1 = W + 1;
        stage_pair_geo(X, geo, W1 * W1, nt, [&](const int p, int &i, int &j) { return pair_of_square(c, W1, p, i, j); });
        PH(41);
        if (be.has_prior) {
            // The prior is kept as the quadratic form (A, b, c0) = (J^T J, J^T r, |r|^2) of the reference's linearised factor:
            // 1/2 |r + J dx|^2 = 1/2 c0 + dx^T b + 1/2 dx^T A dx.  srp receives the gradient q = b + A dx (what assemble / marg add to g).
            matvec_pass(c.prior_H, n, n, n, nullptr, sdx, nullptr, srp, nullptr);  // A dx: one wavefront per row
            for (int i = t; i < n; i += nt) {
                const double b0 = c.prior_r[i], q = b0 + srp[i];
                srp[i] = q;
                cost += 0.5 * sdx[i] * (b0 + q);
            }
            if (t == 0) cost += 0.5 * be.prior_c0;
        }
        const double *ricm = geo + (size_t)W1 * W1 * 32;
#pragma unroll 2
        for (int r = t; r < nres; r += nt) {
            int slot = c.res_lm[r], k = c.res_k[r];
            int imu_i = c.lm_start[slot], imu_j = imu_i + k;
            const bf::PairGeo &g = *(const bf::PairGeo *)(geo + (size_t)(imu_i * W1 + imu_j) * 32);
            double rr[2], wgt = 1.0;
            double sq;
            if (vext) {
                double *out = c.res + (size_t)r * 42;
                bf::eval_projection_pair(cfg, g, ricm, X.ex, feat[c.lm_pidx[slot]], X.td, c.K->tr, obs_ptr(c, slot, imu_i), obs_ptr(c, slot, imu_j),
                                         cfg.estimate_td != 0, rr, withJ ? out : nullptr, true, &wgt);
                sq = rr[0] * rr[0] + rr[1] * rr[1];
                if (withJ) rec_put_wr(out, false, wgt, rr);
            } else {
                double *out = c.res + (size_t)r * 28;
                bf::eval_projection_pair(cfg, g, ricm, X.ex, feat[c.lm_pidx[slot]], X.td, c.K->tr, obs_ptr(c, slot, imu_i), obs_ptr(c, slot, imu_j),
                                         cfg.estimate_td != 0, rr, withJ ? out : nullptr, true, &wgt, 14, false);
                sq = rr[0] * rr[0] + rr[1] * rr[1];
                if (withJ) rec_put_wr(out, true, wgt, rr);
            }
            cost += 0.5 * log(1.0 + sq);
        }
    }
    PH(44);
    cost = block_sum(cost, sred);
    PH(45);
    return cost;
}

// assemble H (P x P, ld LW), g (vec slot 0), Hpl / Hll / gl from the stored residual Jacobians.
// work: LDS scratch (>= max(W*450, npairs*210) doubles when it fits, see be_solve); pb = frame-pair blocks (LDS or HBM)
__device__ __forceinline__ void assemble(const Batch &B, const Ctx &c, const Params &X, int nres, int Fa, const int *alist, double *srp, double *work,
                         double *pb, bool hpl_sparse, bool vext) {
    const int s = c.s;
    PH_INIT;
    const int t = threadIdx.x, nt = blockDim.x, W = c.W, P = c.P, LW = c.LW, n = c.NPR;
    const int lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const BeSeq &be = *c.be;
    double *H = c.H, *g = c.vec;
    for (int i = t; i < P * LW; i += nt) H[i] = 0;
    for (int i = t; i < LW; i += nt) g[i] = 0;
    {
        // landmark rows: with the column-aware Schur staging and mat-vecs (hpl_sparse) only the column tiles that hold pose or
        // extrinsic / td columns are ever read, the speed-bias columns in between need no zeros (the marginalisation kernel uses
        // this buffer as scratch, so they do hold garbage); the dense fall-back paths read whole rows
        // (with constant extrinsic / td blocks and the column-aware paths the extrinsic tile is never read either)
        const int w0 = hpl_sparse ? min(LW, (6 * (W + 1) + 15) & ~15) : LW, e_lo = max(w0, (15 * (W + 1)) & ~15),
                  wz = w0 + ((hpl_sparse && !vext) ? 0 : (LW - e_lo));
        for (int i = t; i < ((Fa + 3) & ~3) * wz; i += nt) {
            const int row = i / wz, cc = i - row * wz;
            c.Hpl[(size_t)row * LW + (cc < w0 ? cc : e_lo + (cc - w0))] = 0;
        }
    }
    __syncthreads();
    PH(32);
    // prior: H += J^T J (precomputed), g += J^T r
    if (be.has_prior) {
        for (int w = t; w < n * n; w += nt) {
            int a = w / n, b = w - a * n;
            H[prior_map(a, W) * LW + prior_map(b, W)] = c.prior_H[w];
        }
        for (int a = t; a < n; a += nt) g[prior_map(a, W)] = srp[a];  // prior gradient b + A dx (computed by evaluate)
    }
    __syncthreads();
    PH(33);
    // IMU: one wavefront per factor.  [J r] (15 x 31, r already whitened by evaluate) is whitened with M = chol(cov)^-1 from a
    // per-wave LDS slice and squared on the FP64 matrix cores (K = 16, three 16x16 accumulators); even factors first, then odd
    // ones (neighbouring factors share the pose / speed-bias block of the frame between them).
    {
        const int li = lane & 15, lk = lane >> 4;
        const int nconc = max(1, min(nw, (W * 450) / 704));
        for (int parity = 0; parity < 2; parity++) {
            for (int base = 0; 2 * base + parity < W; base += nconc) {
                const int i = 2 * (base + wave) + parity;
                bool act = wave < nconc && i < W;
                const PreInt *pp = act ? &c.pre[be.pre_idx[i + 1]] : nullptr;
                if (act && (!c.C->c.use_imu || bf::imu_solver_skips(*pp))) act = false;
                double *raw_l = work + (wave < nconc ? wave : 0) * 704, *M_l = raw_l + 472;
                if (act) {
                    const double *raw = c.imu_raw + (size_t)i * 15 * 31;
                    for (int q = lane; q < 465; q += 64) raw_l[q] = raw[q];
                    for (int q = lane; q < 225; q += 64) M_l[q] = pp->sqrt_info[q];
                }
                __syncthreads();
                if (act) {
                    v4f64 a00 = {0, 0, 0, 0}, a10 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
                    imu_block_mfma(raw_l, M_l, li, lk, a00, a10, a11);
                    auto gidx = [&](int a) {
                        return a < 6 ? 6 * i + a : (a < 15 ? 6 * (W + 1) + 9 * i + (a - 6) : (a < 21 ? 6 * (i + 1) + (a - 15) : 6 * (W + 1) + 9 * (i + 1) + (a - 21)));
                    };
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = lk + 4 * r, col = li;  // C/D layout: acc[r] = element (row, col)
                        const int ic = gidx(col);
                        H[gidx(row) * LW + ic] += a00[r];
                        const int r1 = 16 + row, c1 = 16 + col;
                        if (r1 < 30) {
                            const int ir = gidx(r1);
                            H[ir * LW + ic] += a10[r];
                            H[ic * LW + ir] += a10[r];
                            if (c1 < 30) H[ir * LW + gidx(c1)] += a11[r];
                        } else if (r1 == 30) {
                            g[ic] += a10[r];
                            if (c1 < 30) g[gidx(c1)] += a11[r];
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
    PH(34);
    // vision: frame-pair blocks G_p = [J19 r]^T [J19 r] (packed symmetric 20x20) on the FP64 matrix cores:
    // one wavefront per frame pair, K = 2 rows per residual, three 16x16 accumulators (cols 0-15 / 16-19 of the 20 columns)
    const int W1 = W + 1;
    {
        const int li = lane & 15, lk = lane >> 4;
        for (int p = wave; p < W1 * W1; p += nw) {
            int i = p / W1, j = p - i * W1;
            if (!(i < j)) continue;
            const int q0 = c.pair_start[p], np_ = c.pair_start[p + 1] - q0;
            double *out = pb + (size_t)pair_slot(i, j, W1) * 210;
            if (np_ == 0) { for (int e = lane; e < 210; e += 64) out[e] = 0; continue; }
            v4f64 a00 = {0, 0, 0, 0}, a10 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
            const int K = 2 * np_;
            // residual indices of the pair are fetched 64 at a time (one coalesced load) and broadcast with shuffles; the
            // k loop is unrolled by PB_U with unconditional (clamped) loads so that 2 * PB_U row loads are in flight per MFMA
            // batch: the phase is bound by the L2 latency of those loads (a typical pair is one or two batches), not by the MFMAs
            if (vext) {
                for (int base = 0; base < np_; base += 64) {
                    const int nchunk = min(64, np_ - base);
                    const int myidx = c.pair_list[q0 + base + min(lane, nchunk - 1)];
                    const int Kc = 2 * nchunk;
                    for (int k0 = 0; k0 < Kc; k0 += 4 * PB_U) {
                        double x0[PB_U], x1[PB_U];
#pragma unroll
                        for (int u = 0; u < PB_U; u++) {
                            int kk = k0 + 4 * u + lk;
                            bool valid = kk < Kc;
                            int ridx = __shfl(myidx, min(kk, Kc - 1) >> 1, 64);
                            const double *Jr = c.res + (size_t)ridx * 42;
                            int sub = kk & 1, ro = sub * 20;
                            double v0 = Jr[ro + li];
                            double v1 = Jr[li < 3 ? ro + 16 + li : 40 + sub];
                            x0[u] = valid ? v0 : 0.0;
                            x1[u] = (valid && li < 4) ? v1 : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < PB_U; u++) {
                            if (k0 + 4 * u >= Kc) break;  // wavefront-uniform: the remaining k groups of this batch are all padding
                            a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], x0[u], a00, 0, 0, 0);
                            a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], x0[u], a10, 0, 0, 0);
                            a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], x1[u], a11, 0, 0, 0);
                        }
                    }
                }
                for (int r = 0; r < 4; r++) {
                    int row = lk + 4 * r, col = li;  // C/D layout of v_mfma_f64_16x16x4_f64
                    if (col <= row) out[sym_idx(col, row)] = a00[r];
                    if (row < 4) out[sym_idx(col, 16 + row)] = a10[r];
                    if (row < 4 && col < 4 && col <= row) out[sym_idx(16 + col, 16 + row)] = a11[r];
                }
            } else {
                // compact records: 12 pose columns + the weighted residual in one 16-wide operand (columns 13 .. 15 are padding), one
                // accumulator.  Every output element is the same dot product, in the same k order, as in the three-accumulator form.
                for (int base = 0; base < np_; base += 64) {
                    const int nchunk = min(64, np_ - base);
                    const int myidx = c.pair_list[q0 + base + min(lane, nchunk - 1)];
                    const int Kc = 2 * nchunk;
                    for (int k0 = 0; k0 < Kc; k0 += 4 * PB_U) {
                        double x0[PB_U];
#pragma unroll
                        for (int u = 0; u < PB_U; u++) {
                            int kk = k0 + 4 * u + lk;
                            bool valid = kk < Kc;
                            int ridx = __shfl(myidx, min(kk, Kc - 1) >> 1, 64);
                            const double *Jr = c.res + (size_t)ridx * 28 + (kk & 1) * 14;
                            double v0 = Jr[li < 12 ? li : 13];
                            x0[u] = (valid && li < 13) ? v0 : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < PB_U; u++) {
                            if (k0 + 4 * u >= Kc) break;
                            a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], x0[u], a00, 0, 0, 0);
                        }
                    }
                }
                for (int r = 0; r < 4; r++) {
                    int row = lk + 4 * r, col = li;
                    if (row < 12) { if (col <= row) out[sym_idx(col, row)] = a00[r]; }
                    else if (row == 12 && col <= 12) out[sym_idx(col < 12 ? col : 19, 19)] = a00[r];   // (column, residual) and (residual, residual)
                }
            }
        }
    }
    __syncthreads();
    PH(35);
    {
        // one item per unordered pair (ra <= rb) of vision rows plus one per gradient entry: H is symmetric and both mirror
        // elements receive the same sum (identical terms in identical order), so only half of the element sums are formed
        const int nv = 6 * W1 + (vext ? 7 : 0), ntri = nv * (nv + 1) / 2;   // constant extrinsic / td blocks get no entries at all
        for (int w = t; w < ntri + nv; w += nt) {
            int ra, rb;
            if (w < ntri) {
                int r = (int)((sqrtf(8.0f * (float)w + 1.0f) - 1.0f) * 0.5f);
                while (r * (r + 1) / 2 > w) r--;
                while ((r + 1) * (r + 2) / 2 <= w) r++;
                rb = r; ra = w - r * (r + 1) / 2;
            } else { ra = w - ntri; rb = nv; }
            int a = ra < 6 * W1 ? ra : 15 * W1 + (ra - 6 * W1);
            int b = rb < nv ? (rb < 6 * W1 ? rb : 15 * W1 + (rb - 6 * W1)) : -1;
            double sacc = 0;
            const int fa = ra < 6 * W1 ? ra / 6 : -1, fb = (rb < 6 * W1) ? rb / 6 : -1;
            if (fa >= 0 && fb >= 0 && fa != fb) {
                int i = min(fa, fb), j = max(fa, fb);
                sacc = pb[(size_t)pair_slot(i, j, W1) * 210 + sym_idx(local_of(a, i, j, W), local_of(b, i, j, W))];
            } else if (fa >= 0 || fb >= 0) {
                // diagonal pose block, or pose x (extrinsic / td / gradient): only the W pairs that contain that frame
                const int f = fa >= 0 ? fa : fb;
                for (int o = 0; o < W1; o++) {
                    if (o == f) continue;
                    int i = min(f, o), j = max(f, o);  // empty pairs hold a zero block (written above): no test, no HBM load here
                    int la = local_of(a, i, j, W);
                    int lb = b >= 0 ? local_of(b, i, j, W) : 19;
                    sacc += pb[(size_t)pair_slot(i, j, W1) * 210 + sym_idx(la, lb)];
                }
            } else {
                for (int i = 0; i < W1; i++)
                    for (int j = i + 1; j < W1; j++) {
                        int la = local_of(a, i, j, W);
                        int lb = b >= 0 ? local_of(b, i, j, W) : 19;
                        sacc += pb[(size_t)pair_slot(i, j, W1) * 210 + sym_idx(la, lb)];
                    }
            }
            if (b >= 0) {
                H[a * LW + b] += sacc;
                if (a != b) H[b * LW + a] += sacc;
            } else
                g[a] += sacc;
        }
    }
    PH(36);
    // landmark coupling rows (dense, zero padded above), Hll, gl: two threads per variable landmark walk its residuals; the even one
    // owns the pose columns (start frame + observing frames), the odd one the extrinsic / td columns, Hll and gl
    for (int w = t; w < 2 * Fa; w += nt) {
        const int ka = w >> 1, half = w & 1;
        const int slot = alist[ka];
        const int st = c.lm_start[slot], r0 = c.lm_tmp[slot];
        const int kend = min(c.lm_nobs[slot], nres - r0 + 1);  // residual r0 + k - 1 of observation k, capped by the residual list
        if (vext) lm_row(c.res + (size_t)r0 * 42, c.Hpl + (size_t)ka * LW, c.Hll + ka, c.gl + ka, half, st, kend, 15 * W1);
        else lm_row_compact(c.res + (size_t)r0 * 28, c.Hpl + (size_t)ka * LW, c.Hll + ka, c.gl + ka, half, st, kend);
    }
    __syncthreads();
    PH(37);
}

}  // namespace

// solve -> marginalise -> window slide for one sequence per workgroup (1024 threads); fusing the three stages makes the
// step time the maximum over sequences of the *sum* of the stage times instead of the sum of per-stage maxima.
__device__ __forceinline__ void solve_body(const Batch &B, int s, int *scratch, double *sred, unsigned char *smem, PreWork &pw) {
    const int t = threadIdx.x, nt = blockDim.x;
    Ctx c = make_ctx(B, s);
    const DevCfg &C = *B.cfg;
    const vio_config &cfg = C.c;
    BeSeq &be = *c.be;
    if (!be.do_solve) return;
    const int W = c.W, P = c.P, LW = c.LW, W1 = W + 1;
    __shared__ Params X, Xc;
    __shared__ double sdx[6 * VIO_MAXW + 16], srp[6 * VIO_MAXW + 16];
    __shared__ int sh_i[8];
    __shared__ double sh_d[8];
    double *xs = (double *)smem;  // LW doubles: triangular-solve workspace
    double *work = xs + LW;       // LDS scratch: whitened IMU Jacobians, then the frame-pair blocks
    const int npairs = (W + 1) * W / 2;
    double *pb = (npairs * 210 <= 12288) ? work : c.pairblk;  // 55 pairs x 210 doubles = 92 KB for W = 10
    __shared__ double chol_dinv[VIO_LWMAX];  // reciprocal Cholesky diagonal (LDS-tile path)
    const bool tiles_in_lds = ((LW >> 4) * ((LW >> 4) + 1) / 2) * 256 <= 16896 && !(B.flags & 1);  // S as 66 lower tiles = 132 KB for W = 10
    // column-aware Schur staging (schur_mfma_staged) and two-range Hpl mat-vecs in use: see assemble() / the solver loop
    const bool schur_staged = tiles_in_lds && schur_staged_ok(LW, nt);
    const bool hpl_sparse = schur_staged && 6 * W1 + 7 <= 128;

    PH_INIT;
    const long long ts0 = VIO_CLOCK();
    int F, Fa, nres;
    solve_prologue(B, c, X, scratch, pw, sh_i, F, Fa, nres);
    {
        // The persistent solver (VIO_SOLVE_MODE=0 and the fallback for residual counts beyond the phased solver's range) honours the inverse-depth
        // bound by clamping candidates only; Ceres' treatment of the bounds-constrained program (projection of x0, Armijo line search) lives in
        // the phased solver (be_phased.h).  A frame that meets a bounded landmark here is flagged (overflow bit 512: a deviation from the
        // reference, not lost capacity), and the bounded landmarks / clamped candidates are counted as ps_setup / ps_form_candidate count them
        // (vio_get_bound_stats; no line search runs here, its two counters stay 0)
        const int *al = c.pair_list + c.nres_cap - c.NL;
        int nb = 0;
        for (int k = t; k < Fa; k += nt) nb += c.lm_est[al[k]] == 2 ? 1 : 0;
        if (nb) { atomicOr(&c.be->overflow, 512); atomicAdd(&c.be->bounded_solves, nb); }
    }
    const int nlm = be.n_lm;
    int *alist = c.pair_list + c.nres_cap - c.NL;              // variable-landmark slots, kept for the whole solve
    const int n = c.NPR;
    PH(2);
    const int ex_active = sh_i[0], td_active = sh_i[1];
    const bool vext = ex_active || td_active;   // extrinsic / td Jacobians are only evaluated when one of the blocks is a variable
    const int ne_ext = vext ? 7 : 0;
    const int oE = 15 * W1, oT = 15 * W1 + 6;

    // vec slots
    double *g = c.vec, *sp = c.vec + 1 * LW, *dgp = c.vec + 2 * LW, *gradp = c.vec + 3 * LW, *gnp = c.vec + 4 * LW, *stp = c.vec + 5 * LW,
           *gs = c.vec + 6 * LW, *tmpv = c.vec + 7 * LW, *delta = c.vec + 8 * LW, *sgp = c.vec + 9 * LW, *hsgp = c.vec + 10 * LW,
           *yp = c.vec + 11 * LW, *up = c.vec + 12 * LW, *tmpv2 = c.vec + 13 * LW;
    double *sl = c.lvec, *dgl = c.lvec + c.NLs, *gradl = c.lvec + 2 * c.NLs, *gnl = c.lvec + 3 * c.NLs, *stl = c.lvec + 4 * c.NLs,
           *inv = c.lvec + 5 * c.NLs, *gls = c.lvec + 6 * c.NLs, *Hlls = c.lvec + 7 * c.NLs;
    const int Kpad = (Fa + 3) & ~3;
    double *hsgl = c.res + (size_t)c.nres_cap * 42 - 4 * (size_t)c.NLs;   // tail of the residual buffer (nres <= nres_cap - 2 NL)
    double *yl = hsgl + c.NLs, *ul = yl + c.NLs, *tmpl = ul + c.NLs;

    double cost = evaluate(c, X, c.feat, true, nres, sred, sdx, srp, work, vext);
    PH(4);
    assemble(B, c, X, nres, Fa, alist, srp, work, pb, hpl_sparse, vext);
    PH(5);
    if (t == 0) be.initial_cost = cost;
    // Jacobi scaling (once): 1/(1+||J_j||); constant blocks (ex / td when not estimated) get scale 0 = removed from the problem
    for (int a = t; a < LW; a += nt) {
        bool act = a < P && (a < oE ? true : (a < oT ? ex_active != 0 : td_active != 0));
        if (!cfg.use_imu && (a < 6 || (a >= 6 * W1 && a < oE))) act = false;   // VO mode: pose 0 constant, no speed-bias blocks (estimator.cpp:1178-1185)
        sp[a] = act ? 1.0 / (1.0 + sqrt(c.H[a * LW + a])) : 0.0;
    }
    for (int k = t; k < Kpad; k += nt) sl[k] = k < Fa ? 1.0 / (1.0 + sqrt(c.Hll[k])) : 0.0;
    __syncthreads();
    // H / Hpl stay unscaled in HBM; the column scaling S is applied to the vectors (and inside the Schur MFMA operand loads):
    //   Hs v = S H (S v).  Returns the max-norm of the active gradient.
    auto prepare_point = [&]() -> double {
        double m = 0;
        for (int a = t; a < P; a += nt) m = fmax(m, sp[a] != 0.0 ? fabs(g[a]) : 0.0);
        for (int k = t; k < Fa; k += nt) m = fmax(m, fabs(c.gl[k]));
        double r = block_max(m, sred);
        for (int a = t; a < LW; a += nt) {
            double hs = a < P ? sp[a] * sp[a] * c.H[a * LW + a] : 0.0;
            gs[a] = a < P ? sp[a] * g[a] : 0.0;
            dgp[a] = sqrt(fmin(fmax(hs, 1e-6), 1e32));
            gradp[a] = gs[a] / dgp[a];
            sgp[a] = gradp[a] / dgp[a];
            up[a] = sp[a] * sgp[a];
        }
        for (int k = t; k < Kpad; k += nt) {
            double hl = k < Fa ? sl[k] * sl[k] * c.Hll[k] : 0.0;
            Hlls[k] = hl;
            gls[k] = k < Fa ? sl[k] * c.gl[k] : 0.0;
            dgl[k] = sqrt(fmin(fmax(hl, 1e-6), 1e32));
            gradl[k] = gls[k] / dgl[k];
            ul[k] = sl[k] * (gradl[k] / dgl[k]);
        }
        __syncthreads();
        return r;
    };

    double radius = 1e4, mu = 1e-8, alpha = 0, dogleg_norm = 0;
    // Cauchy point, computed lazily: the dogleg only needs it when the Gauss-Newton step leaves the trust region (rare with the
    // initial radius 1e4).  It depends on H, g only, which stay valid until the next assemble(); the LDS work region is free then.
    bool cauchy_valid = false;
    auto compute_cauchy = [&]() {
        // Cauchy point: alpha = |grad|^2 / |J D^-1 grad|^2, and H_full * (D^-1 grad) is kept for the model evaluation
        matvec_pass(c.H, LW, P, P, nullptr, up, nullptr, tmpv, work);   // H (S sg_p): H is symmetric, row dots
        matvec_pass_2range(c.Hpl, LW, Fa, P, 6 * W1, 15 * W1, ne_ext, ul, up, tmpv2, tmpl, work);       // Hpl^T (Sl sg_l) and Hpl (S sg_p) in one pass
        double g2 = 0, jg2 = 0;
        for (int a = t; a < LW; a += nt) {
            double v = a < P ? sp[a] * (tmpv[a] + tmpv2[a]) : 0.0;
            hsgp[a] = v;
            if (a < P) { g2 += gradp[a] * gradp[a]; jg2 += sgp[a] * v; }
        }
        for (int k = t; k < Kpad; k += nt) {
            double sgl = k < Fa ? gradl[k] / dgl[k] : 0.0;
            double v = k < Fa ? sl[k] * tmpl[k] + Hlls[k] * sgl : 0.0;
            hsgl[k] = v;
            if (k < Fa) { g2 += gradl[k] * gradl[k]; jg2 += sgl * v; }
        }
        block_sum2(g2, jg2, sred);
        alpha = g2 / jg2;
        cauchy_valid = true;
    };

    bool reuse = false, need_eval = false, have_J = false;
    int invalid = 0;
    int iters_done = 0, succ = 0;
    if (prepare_point() > 1e-10)
    for (int iter = 1; iter <= cfg.max_iterations; iter++) {
        iters_done = iter;
        if (!reuse) {
            if (need_eval) {
                PH(13);
                if (!have_J) cost = evaluate(c, X, c.feat, true, nres, sred, sdx, srp, work, vext);
                have_J = false;
                PH(4);
                assemble(B, c, X, nres, Fa, alist, srp, work, pb, hpl_sparse, vext);
                PH(5);
                need_eval = false;
                if (prepare_point() <= 1e-10) { iters_done = iter - 1; break; }
                PH(6);
            }
            cauchy_valid = false;
            // Gauss-Newton step via the landmark Schur complement (FP64 matrix cores), regularised by mu * D^2
            bool ok = false;
            while (mu < 1.0) {
                for (int k = t; k < Kpad; k += nt) {
                    double iv = k < Fa ? 1.0 / (Hlls[k] + mu * dgl[k] * dgl[k]) : 0.0;
                    inv[k] = iv;
                    tmpl[k] = sl[k] * iv * gls[k];
                }
                __syncthreads();
                matvec_pass_2range(c.Hpl, LW, Fa, P, 6 * W1, 15 * W1, ne_ext, tmpl, nullptr, tmpv, nullptr, work);  // Hpl^T (Sl gls / hll); uses the work region before S moves in
                for (int a = t; a < LW; a += nt) xs[a] = a < P ? gs[a] - sp[a] * tmpv[a] : 0.0;
                for (int k = t; k < Kpad; k += nt) tmpl[k] = sl[k] * sl[k] * inv[k];  // per-row factor of the rank-K update
                __syncthreads();
                bool chol_ok;
                if (tiles_in_lds) {
                    {
                        // column tiles of Hpl that can be non-zero: poses (columns 0 .. 6 W1 - 1) and extrinsic / td (15 W1 .. 15 W1 + 6)
                        unsigned colmask = 0;
                        for (int cb = 0; cb < (LW >> 4); cb++) {
                            const int c0 = 16 * cb, c1 = c0 + 15;
                            if (c0 < 6 * W1 || (vext && c1 >= 15 * W1 && c0 < 15 * W1 + 7)) colmask |= 1u << cb;
                        }
                        if (schur_staged)
                            schur_mfma_staged<9>(c.H, c.Hpl, tmpl, dgp, sp, mu, Kpad, LW, LW, work, colmask);
                        else schur_mfma_lds(c.H, c.Hpl, tmpl, dgp, sp, mu, Kpad, LW, LW, work);
                    }
                    PH(8);
                    chol_ok = chol_tiles(work, LW >> 4, &sh_i[2], chol_dinv, nullptr, xs);   // with the forward substitution
                } else {
                    schur_mfma(c.H, c.Hpl, tmpl, dgp, sp, mu, Kpad, LW, LW, c.Sc);
                    PH(8);
                    chol_ok = chol_blocked(c.Sc, LW, LW, &sh_i[2], work);
                }
                PH(9);
                if (chol_ok) {
                    if (tiles_in_lds) chol_backward_tiles_wave(work, LW >> 4, xs, chol_dinv);
                    else chol_solve_blocked(c.Sc, LW, LW, xs, work);
                    PH(10);
                    double bad = 0;
                    for (int a = t; a < P; a += nt) if (!isfinite(xs[a])) bad += 1;
                    bad = block_sum(bad, sred);
                    if (bad == 0) {
                        for (int a = t; a < LW; a += nt) { yp[a] = xs[a]; gnp[a] = -xs[a] * dgp[a]; tmpv[a] = sp[a] * xs[a]; }
                        __syncthreads();
                        matvec_pass_2range(c.Hpl, LW, Fa, P, 6 * W1, 15 * W1, ne_ext, nullptr, tmpv, nullptr, tmpl, nullptr);  // Hpl (S y_p)
                        for (int k = t; k < Kpad; k += nt) {
                            double y = k < Fa ? (gls[k] - sl[k] * tmpl[k]) * inv[k] : 0.0;
                            yl[k] = y;
                            gnl[k] = -y * dgl[k];
                        }
                        __syncthreads();
                        ok = true;
                        break;
                    }
                }
                mu *= 10.0;
            }
            if (!ok) break;
            reuse = true;
        }
        // traditional dogleg in the D-scaled space
        double gnorm = 0, gnn = 0, gdot = 0;
        for (int a = t; a < P; a += nt) { gnorm += gradp[a] * gradp[a]; gnn += gnp[a] * gnp[a]; gdot += gradp[a] * gnp[a]; }
        for (int k = t; k < Fa; k += nt) { gnorm += gradl[k] * gradl[k]; gnn += gnl[k] * gnl[k]; gdot += gradl[k] * gnl[k]; }
        block_sum3(gnorm, gnn, gdot, sred);
        gnorm = sqrt(gnorm);
        gnn = sqrt(gnn);
        double ca = 0, cb = 0;  // step = ca * grad + cb * gn
        if (!(gnn <= radius) && !cauchy_valid) { PH(11); compute_cauchy(); PH(7); }
        if (gnn <= radius) { ca = 0; cb = 1; dogleg_norm = gnn; }
        else if (gnorm * alpha >= radius) { ca = -(radius / gnorm); cb = 0; dogleg_norm = radius; }
        else {
            double b_dot_a = -alpha * gdot;
            double a_sq = (alpha * gnorm) * (alpha * gnorm);
            double bma = a_sq - 2 * b_dot_a + gnn * gnn;
            double cc = b_dot_a - a_sq;
            double d = sqrt(cc * cc + bma * (radius * radius - a_sq));
            double beta = (cc <= 0) ? (d - cc) / bma : (radius * radius - a_sq) / (d + cc);
            ca = -alpha * (1.0 - beta); cb = beta;
            dogleg_norm = -1;
        }
        // step = ca * D^-1 grad - cb * y ;  H_full step = ca * H_full (D^-1 grad) - cb * (g' - mu D^2 y)   [(H_full + mu D^2) y = g']
        double n2 = 0, lin = 0, quad = 0;
        for (int a = t; a < LW; a += nt) {
            double v = ca * gradp[a] + cb * gnp[a];
            double st = a < P ? v / dgp[a] : 0.0;
            stp[a] = st;
            if (a < P) {
                n2 += v * v;
                lin += st * gs[a];
                quad += st * ((ca != 0.0 ? ca * hsgp[a] : 0.0) - cb * (gs[a] - mu * dgp[a] * dgp[a] * yp[a]));
            }
        }
        for (int k = t; k < Kpad; k += nt) {
            double v = k < Fa ? ca * gradl[k] + cb * gnl[k] : 0.0;
            double st = k < Fa ? v / dgl[k] : 0.0;
            stl[k] = st;
            if (k < Fa) {
                n2 += v * v;
                lin += st * gls[k];
                quad += st * ((ca != 0.0 ? ca * hsgl[k] : 0.0) - cb * (gls[k] - mu * dgl[k] * dgl[k] * yl[k]));
            }
        }
        block_sum3(n2, lin, quad, sred);
        if (dogleg_norm < 0) dogleg_norm = sqrt(n2);
        double model_change = -(lin + 0.5 * quad);
        PH(11);
        if (!(model_change > 0)) {
            if (++invalid >= 5) break;
            mu *= 10.0;
            reuse = false;
            continue;
        }
        invalid = 0;
        // candidate = Plus(x, step .* scale)
        for (int a = t; a < P; a += nt) delta[a] = stp[a] * sp[a];
        __syncthreads();
        if (t <= W) {
            for (int k = 0; k < 7; k++) Xc.pose[t * 7 + k] = X.pose[t * 7 + k];
            bf::pose_plus(&Xc.pose[t * 7], &delta[6 * t]);
            for (int k = 0; k < 9; k++) Xc.sb[t * 9 + k] = X.sb[t * 9 + k] + delta[6 * W1 + 9 * t + k];
        }
        if (t == W + 1) {
            for (int k = 0; k < 7; k++) Xc.ex[k] = X.ex[k];
            if (ex_active) bf::pose_plus(Xc.ex, &delta[oE]);
            Xc.td = X.td + (td_active ? delta[oT] : 0.0);
        }
        for (int k = t; k < F; k += nt) c.cfeat[k] = c.feat[k];
        __syncthreads();
        for (int k = t; k < Fa; k += nt) {
            int slot = alist[k], pi = c.lm_pidx[slot];
            double v = c.feat[pi] + stl[k] * sl[k];
            double ub = (c.lm_est[slot] == 2) ? 2.0 / cfg.depth_max : 1.7976931348623157e308;
            if (v > ub) { v = ub; atomicAdd(&be.bound_clamps, 1); }
            c.cfeat[pi] = v;
        }
        __syncthreads();
        // The candidate is evaluated WITH Jacobians (res / imu_raw / srp are only read by assemble(), which is not called again if the
        // step is rejected): an accepted point then goes straight to assemble() instead of being evaluated a second time.
        const bool cand_with_J = iter < cfg.max_iterations;
        double ccost = evaluate(c, Xc, c.cfeat, cand_with_J, nres, sred, sdx, srp, work, vext);
        PH(12);
        // parameter tolerance
        double xn = 0, dn = 0;
        if (t <= W) {
            for (int k = 0; k < 7; k++) { double v = X.pose[t * 7 + k]; xn += v * v; double d = v - Xc.pose[t * 7 + k]; dn += d * d; }
            for (int k = 0; k < 9; k++) { double v = X.sb[t * 9 + k]; xn += v * v; double d = v - Xc.sb[t * 9 + k]; dn += d * d; }
        }
        if (t == W + 1) {
            if (ex_active) for (int k = 0; k < 7; k++) { double v = X.ex[k]; xn += v * v; double d = v - Xc.ex[k]; dn += d * d; }
            if (td_active) { xn += X.td * X.td; dn += (X.td - Xc.td) * (X.td - Xc.td); }
        }
        for (int k = t; k < Fa; k += nt) { int pi = c.lm_pidx[alist[k]]; double v = c.feat[pi]; xn += v * v; double d = v - c.cfeat[pi]; dn += d * d; }
        block_sum2(xn, dn, sred);
        if (sqrt(dn) <= 1e-8 * (sqrt(xn) + 1e-8)) break;
        if (fabs(cost - ccost) <= 1e-6 * cost) break;
        double rel = (cost - ccost) / model_change;
        if (rel > 1e-3) {
            __syncthreads();
            if (t <= W) { for (int k = 0; k < 7; k++) X.pose[t * 7 + k] = Xc.pose[t * 7 + k]; for (int k = 0; k < 9; k++) X.sb[t * 9 + k] = Xc.sb[t * 9 + k]; }
            if (t == W + 1) { for (int k = 0; k < 7; k++) X.ex[k] = Xc.ex[k]; X.td = Xc.td; }
            for (int k = t; k < F; k += nt) c.feat[k] = c.cfeat[k];
            __syncthreads();
            cost = ccost;
            succ++;
            if (rel < 0.25) radius *= 0.5;
            if (rel > 0.75) radius = fmax(radius, 3.0 * dogleg_norm);
            mu = fmax(1e-8, 2.0 * mu / 10.0);
            reuse = false;
            need_eval = true;
            have_J = cand_with_J;
        } else {
            radius *= 0.5;
            reuse = true;
        }
    }
    __syncthreads();
    PH(13);
    solve_epilogue(c, X, cost, iters_done, succ, ts0, sdx, sh_d, sh_i);
}

// ====================================================================================================== be_marg
// Marginalisation in the canonical layout. Landmarks seen first in frame 0 are eliminated analytically (their block of
// A_mm is diagonal), then pose_0/speedbias_0 (15) through a truncated eigen-decomposition, then the kept block is
// re-factorised as J^T J by a second (parallel Jacobi) eigen-decomposition (marginalization_factor.cpp:276-308).
// marg_exact (vio_config): elimination of the marginalised block and the new prior exactly as MarginalizationInfo::marginalize does them
// (marginalization_factor.cpp:270-315).  In: A (mq x mq over q = [md | n]) and b with NO landmark eliminated, the landmark coupling rows
// Cl (F0 x ldc, columns indexed like q), d_l = c.Hll (J_l^T J_l), c.gl (J_l^T r).  Marginalised block: m = md + F0 = [pose 0, speed-bias 0
// | inverse depths of the landmarks that start in frame 0] (md = 6 and F0 = 0 for MARGIN_SECOND_NEW).  Both eigen-decompositions are Householder
// tridiagonalisation + implicit QL: LDS-resident where the block fits (sym_eig_lds), on the matrix in HBM scratch otherwise (sym_eig_hbm).
// LDS layout of the literal marginalisation's eigen-decompositions: the matrix (ld = n | 1: conflict-free column access), then d / e / g and
// the per-wavefront partial sums of sym_eig_tridiag_mt.  Host side: marg_exact_lds_bytes (kernels.h) sizes the launch with the same formula.
#define MARG_EIG_AUX_DOUBLES (11 * EIG_LD)
static_assert(MARG_EXACT_HBM_LDS_DOUBLES == SYM_EIG_HBM_LDS_DOUBLES, "kernels.h marg_exact_hbm_lds_bytes: the host sizes sym_eig_hbm's LDS");
// Symmetric eigen-decomposition in LDS: A (n x n, ld) -> eigenvectors in place (columns), eigenvalues in d.  Householder tridiagonalisation over
// the whole workgroup + implicit QL on one wavefront (be_linalg.h; the same pair be_prior_factor_kernel runs).  n <= 128 (tridiag_ql_wave).
__device__ __forceinline__ void sym_eig_lds(double *Al, int n, int ld, double *aux) {
    double *d = aux, *e = aux + EIG_LD, *g = aux + 2 * EIG_LD, *part = aux + 3 * EIG_LD;
    sym_eig_tridiag_mt(Al, n, ld, d, e, g, part);
    tridiag_ql_wave(Al, n, ld, d, e);
}
// The SECOND half of MarginalizationInfo::marginalize (marginalization_factor.cpp:293-315), literally: saes2(A), S = eigenvalues > 1e-8,
// linearized_jacobians = S^1/2 V^T, linearized_residuals = S^-1/2 V^T b, and from them what the solver consumes (J^T J, J^T r, |r|^2).
// Ar (n x n, HBM) / br (n) = the reduced system.  Householder + implicit QL, LDS-resident when n <= MXL, else on HBM scratch (scrA: n x n for the
// symmetrised matrix, which its eigenvectors replace).
// Not inlined: its own register allocation, one copy in the kernel for both literal modes (marg_exact 1 and 2).
__device__ __noinline__ void marg_literal_prior(const Ctx &c, BeSeq &be, const double *Ar, const double *br, int n, double *scrA, double *sred) {
    const int t = threadIdx.x, nt = blockDim.x;
    const double eps = 1e-8;
    extern __shared__ __attribute__((aligned(16))) unsigned char marg_dyn_lds[];
    __shared__ double ev2[EIG_LD], vb2[EIG_LD];
    if (n <= c.C->MXL) {
        const int ld = n | 1;
        double *Al = (double *)marg_dyn_lds, *aux = Al + (size_t)n * ld;
        for (int w = t; w < n * n; w += nt) { const int i = w / n, j = w - i * n; Al[i * ld + j] = 0.5 * (Ar[i * n + j] + Ar[j * n + i]); }
        __syncthreads();
        sym_eig_lds(Al, n, ld, aux);   // SelfAdjointEigenSolver<MatrixXd> saes2(A) (:298)
        for (int k = t; k < n; k += nt) {
            const double ev = aux[k];
            double vb = 0;
            for (int i = 0; i < n; i++) vb += Al[i * ld + k] * br[i];
            c.prior_rf[k] = sqrt(ev > eps ? 1.0 / ev : 0.0) * vb;
            aux[EIG_LD + k] = sqrt(ev > eps ? ev : 0.0);
        }
        __syncthreads();
        // J = S^1/2 V^T: column k of the eigenvector array scaled in place, so Al[i][k] = J[k][i]
        for (int w = t; w < n * n; w += nt) { const int i = w / n, k = w - i * n; const double v = aux[EIG_LD + k] * Al[i * ld + k]; Al[i * ld + k] = v; c.prior_J[k * n + i] = v; }
        __syncthreads();
        // what MarginalizationFactor::Evaluate, the solver and the next marginalisation consume of (J, r): J^T J, J^T r and |r|^2
        for (int w = t; w < n * n; w += nt) {
            const int a = w / n, bb = w - a * n;
            double sacc = 0;
            for (int k = 0; k < n; k++) sacc += Al[a * ld + k] * Al[bb * ld + k];
            c.prior_H[w] = sacc;
        }
        for (int a = t; a < n; a += nt) {
            double sacc = 0;
            for (int k = 0; k < n; k++) sacc += Al[a * ld + k] * c.prior_rf[k];
            c.prior_r[a] = sacc;
        }
    } else {
        double *As = scrA;
        for (int w = t; w < n * n; w += nt) { const int i = w / n, j = w - i * n; As[w] = 0.5 * (Ar[i * n + j] + Ar[j * n + i]); }
        __syncthreads();
        sym_eig_hbm(As, n, n, (double *)marg_dyn_lds, sred);   // Householder + implicit QL on the matrix where it lies: the eigenvectors replace it
        const double *V2 = As;
        for (int k = t; k < n; k += nt) {
            ev2[k] = ((const double *)marg_dyn_lds)[k];
            double vb = 0;
            for (int i = 0; i < n; i++) vb += V2[i * n + k] * br[i];
            vb2[k] = vb;
        }
        __syncthreads();
        for (int w = t; w < n * n; w += nt) {
            const int k = w / n, i = w - k * n;
            const double S = ev2[k] > eps ? ev2[k] : 0.0;
            c.prior_J[w] = sqrt(S) * V2[i * n + k];
        }
        for (int k = t; k < n; k += nt) {
            const double Sinv = ev2[k] > eps ? 1.0 / ev2[k] : 0.0;
            c.prior_rf[k] = sqrt(Sinv) * vb2[k];
        }
        __syncthreads();
        for (int w = t; w < n * n; w += nt) {
            const int a = w / n, bb = w - a * n;
            double sacc = 0;
            for (int k = 0; k < n; k++) sacc += c.prior_J[k * n + a] * c.prior_J[k * n + bb];
            c.prior_H[w] = sacc;
        }
        for (int a = t; a < n; a += nt) {
            double sacc = 0;
            for (int k = 0; k < n; k++) sacc += c.prior_J[k * n + a] * c.prior_rf[k];
            c.prior_r[a] = sacc;
        }
    }
    __syncthreads();
    double acc = 0;
    for (int k = t; k < n; k += nt) acc += c.prior_rf[k] * c.prior_rf[k];
    const double c0 = block_sum(acc, sred);
    __syncthreads();
    if (t == 0) be.prior_c0 = c0;
}

// Not inlined, like marg_literal_prior: inlined into marg_body the kernel spills 111 VGPRs, with its own register allocation none.
__device__ __noinline__ void marg_exact_finish(const Ctx &c, BeSeq &be, double *A, const double *b, int md, int mq, int n, const double *Cl, int ldc, int F0,
                                  bool second_new, double *sred) {
    const int t = threadIdx.x, nt = blockDim.x;
    const double eps = 1e-8;
    const int MX = c.C->MX, m = md + F0;
    double *Emm = c.margE, *Einv = Emm + 2 * (size_t)MX * MX, *ET1 = Einv + (size_t)MX * MX;   // (A_mm, which its eigenvectors replace; a free block; A_mm^+; A_rm A_mm^+)
    // the dynamic LDS of this kernel, declared here so that the eigen-solver below is compiled for ds_* accesses (a pointer handed down
    // through two calls would be flat); same base address as the caller's smem
    extern __shared__ __attribute__((aligned(16))) unsigned char marg_dyn_lds[];
    // Amm = 0.5 (Amm + Amm^T) (:276); the landmark-landmark block is diagonal (an inverse depth only meets itself)
    auto amm = [&](int i, int j) -> double {
        if (i < md && j < md) return 0.5 * (A[i * mq + j] + A[j * mq + i]);
        if (i >= md && j >= md) return i == j ? c.Hll[i - md] : 0.0;
        return Cl[(size_t)((i >= md ? i : j) - md) * ldc + (i >= md ? j : i)];
    };
    // The first eigen-decomposition (saes(Amm), :281) runs LDS-resident when the block fits (m <= MXL); the second one lives in marg_literal_prior.
    double *Ar = c.margV, *br = c.vec;
    const long long tx0 = VIO_CLOCK();   // (timers build only: dbg[7..10] = ticks to the end of eig 1 / the Schur products / eig 2 / the prior; tools/marg_exact_probe.py)
    if (m <= c.C->MXL) {
        const int ld = m | 1;
        double *Al = (double *)marg_dyn_lds, *aux = Al + (size_t)m * ld;
        for (int w = t; w < m * m; w += nt) { const int i = w / m, j = w - i * m; Al[i * ld + j] = amm(i, j); }
        __syncthreads();
        sym_eig_lds(Al, m, ld, aux);
        if (VIO_TIMERS && t == 0) be.dbg[7] = (int)(VIO_CLOCK() - tx0);
        // Amm_inv = V diag(lambda > eps ? 1 / lambda : 0) V^T (:281-283); 1 / lambda once per column
        for (int k = t; k < m; k += nt) { const double ev = aux[k]; aux[EIG_LD + k] = ev > eps ? 1.0 / ev : 0.0; }
        __syncthreads();
        for (int w = t; w < m * m; w += nt) {
            const int i = w / m, j = w - i * m;
            double sacc = 0;
            for (int k = 0; k < m; k++) sacc += Al[i * ld + k] * Al[j * ld + k] * aux[EIG_LD + k];
            Einv[w] = sacc;
        }
    } else {
        for (int w = t; w < m * m; w += nt) { const int i = w / m, j = w - i * m; Emm[w] = amm(i, j); }
        __syncthreads();
        // Householder + implicit QL on the matrix where it lies (be_linalg.h sym_eig_hbm; 23 ms at m = 185)
        double *ewk = (double *)marg_dyn_lds;
        sym_eig_hbm(Emm, m, m, ewk, sred);
        if (VIO_TIMERS && t == 0) be.dbg[7] = (int)(VIO_CLOCK() - tx0);
        for (int k = t; k < m; k += nt) { const double ev = ewk[k]; ewk[SYM_EIG_HBM_MAX + k] = ev > eps ? 1.0 / ev : 0.0; }
        __syncthreads();
        for (int w = t; w < m * m; w += nt) {   // Amm_inv = V diag(lambda > eps ? 1 / lambda : 0) V^T: rows i and j of V, sixteen columns per trip
            const int i = w / m, j = w - i * m;
            const double *vi = Emm + (size_t)i * m, *vj = Emm + (size_t)j * m;
            double sacc = 0;
            for (int k0 = 0; k0 < m; k0 += 16) {
                double a[16], b[16];
#pragma unroll
                for (int u = 0; u < 16; u++) { const int k = min(k0 + u, m - 1); a[u] = vi[k]; b[u] = vj[k]; }
#pragma unroll
                for (int u = 0; u < 16; u++) if (k0 + u < m) sacc += a[u] * b[u] * ewk[SYM_EIG_HBM_MAX + k0 + u];
            }
            Einv[w] = sacc;
        }
    }
    __syncthreads();
    // A_rm A_mm^-1 (:288-292); column k of A_rm: q-column k for the pose / speed-bias part, the coupling row of landmark k - md otherwise
    for (int w = t; w < n * m; w += nt) {
        const int i = w / m, j = w - i * m;
        double sacc = 0;
        for (int k = 0; k < md; k++) sacc += A[(md + i) * mq + k] * Einv[(size_t)k * m + j];
        for (int k0 = md; k0 < m; k0 += 16) {   // (sixteen terms' loads in flight; same order of the sum)
            double a[16], b[16];
#pragma unroll
            for (int u = 0; u < 16; u++) { const int k = min(k0 + u, m - 1); a[u] = Cl[(size_t)(k - md) * ldc + md + i]; b[u] = Einv[(size_t)k * m + j]; }
#pragma unroll
            for (int u = 0; u < 16; u++) if (k0 + u < m) sacc += a[u] * b[u];
        }
        ET1[w] = sacc;
    }
    __syncthreads();
    for (int w = t; w < n * n; w += nt) {   // A = Arr - Arm Amm_inv Amr
        const int i = w / n, j = w - i * n;
        double tt = A[(md + i) * mq + md + j];
        for (int k = 0; k < md; k++) tt -= ET1[(size_t)i * m + k] * A[k * mq + md + j];
        for (int k0 = md; k0 < m; k0 += 16) {
            double a[16], b[16];
#pragma unroll
            for (int u = 0; u < 16; u++) { const int k = min(k0 + u, m - 1); a[u] = ET1[(size_t)i * m + k]; b[u] = Cl[(size_t)(k - md) * ldc + md + j]; }
#pragma unroll
            for (int u = 0; u < 16; u++) if (k0 + u < m) tt -= a[u] * b[u];
        }
        Ar[w] = tt;
    }
    for (int i = t; i < n; i += nt) {       // b = brr - Arm Amm_inv bmm
        double sacc = b[md + i];
        for (int k = 0; k < md; k++) sacc -= ET1[(size_t)i * m + k] * b[k];
        for (int k = md; k < m; k++) sacc -= ET1[(size_t)i * m + k] * c.gl[k - md];
        br[i] = sacc;
    }
    __syncthreads();
    if (VIO_TIMERS && t == 0) be.dbg[8] = (int)(VIO_CLOCK() - tx0);
    // second eigen-decomposition and the prior (:293-315)
    marg_literal_prior(c, be, Ar, br, n, c.margW, sred);
    if (VIO_TIMERS && t == 0) be.dbg[9] = (int)(VIO_CLOCK() - tx0);
    if (t == 0) { be.dbg[0] = 0; be.dbg[2] = second_new ? 1 : 0; be.dbg[4] = m; }
    if (VIO_TIMERS && t == 0) be.dbg[10] = (int)(VIO_CLOCK() - tx0);
}

// The certificate of marg_exact = 2 (marg_body): |A_mm^-1|_F <= |S^-1|_F + 2 |T|_F + |D^-1|_F + |D^-1 B|_F |T|_F with A_mm = [[P, B^T], [B, D]],
// S = P - B^T D^-1 B (Pinv = S^-1, md x md, LDS), T = S^-1 B^T D^-1; it needs D invertible (every landmark's d > eps) and the direct inverse of S.
// Cl: the rows B (F0k x ldc), Hll: 1 / d.  The whole workgroup calls it; the answer (and *bound_out, if asked for) is thread 0's.
__device__ __forceinline__ bool marg_certificate(const double *Pinv, int md, int pinv_direct, bool second_new, const double *Cl, int ldc, const double *Hll,
                                                 int F0k, double *sred, double *bound_out) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ int cert_bad;
    if (t == 0) cert_bad = pinv_direct ? 0 : 1;
    __syncthreads();
    double n_t = 0, n_d = 0, n_db = 0;
    if (!second_new) {
        for (int li = t; li < F0k; li += nt) {
            const double dinv = Hll[li];             // 1 / d, or 0 where d <= eps (pseudo-inverse of the diagonal block)
            if (!(dinv > 0.0)) cert_bad = 1;         // (benign race: every writer stores 1)
            n_d += dinv * dinv;
            for (int a = 0; a < md; a++) {
                double tt = 0;
                for (int bq = 0; bq < md; bq++) tt += Pinv[a * md + bq] * Cl[(size_t)li * ldc + bq];
                tt *= dinv;
                n_t += tt * tt;
                const double db = dinv * Cl[(size_t)li * ldc + a];
                n_db += db * db;
            }
        }
    }
    block_sum3(n_t, n_d, n_db, sred);
    double n_s = 0;
    for (int w = t; w < md * md; w += nt) n_s += Pinv[w] * Pinv[w];
    n_s = block_sum(n_s, sred);
    __syncthreads();
    bool certified = false;
    if (t == 0) {
        const double bound = sqrt(n_s) + 2.0 * sqrt(n_t) + sqrt(n_d) + sqrt(n_db) * sqrt(n_t);
        certified = !cert_bad && isfinite(bound) && bound > 0.0 && 1.0 / bound > 1e-7;   // ten times the cut
        if (bound_out) *bound_out = bound;
    }
    return certified;
}

// LDSA: the reduced system A, b, b_r and the frame blocks G_j live in the dynamic LDS (kernels.h marg_resident_lds_bytes) instead of c.margA / margB /
// margV / vec / pairblk; LT: the window slide works on LDS copies of the landmark tables.  Compile-time, so that every loop addresses one address space.
// PART (kernels.h MargSnap): 0 = the whole stage, 1 = what must precede the window slide (be_marg_pre_kernel), 2 = the algebra from the hand-over
// record (be_marg_alg_kernel); msnap / mlist: that record and the list of this sequence (PART != 0)
template <bool EXACT, bool LDSA, int PART = 0> __device__ void marg_body(const Batch &B, int s, int *scratch, double *sred, unsigned char *smem_marg,
                                                                     MargSnap *msnap = nullptr, int *mlist = nullptr) {
    static_assert(!(EXACT && LDSA), "the literal marginalisation keeps its system in HBM");
    static_assert(PART == 0 || !EXACT, "the split runs the default marginalisation only");
    const int t = threadIdx.x, nt = blockDim.x;
    Ctx c = make_ctx(B, s);
    const DevCfg &C = *B.cfg;
    const vio_config &cfg = C.c;
    BeSeq &be = *c.be;
    // PART 2 decides nothing itself: the guards below were taken by PART 1, before the slide and the next frame's be_ingest rewrote what they read
    if constexpr (PART == 2) { if (!msnap->active) return; }
    else {
        if (PART == 1 && t == 0) msnap->active = 0;
        if (!be.do_marg || be.rebooted || be.frame_count < c.W) return;
    }
    const int W = c.W, W1 = W + 1, n = c.NPR;
    const double eps = 1e-8;
    __shared__ Params X;
    __shared__ double sdx[6 * VIO_MAXW + 16], srp[6 * VIO_MAXW + 16];
    __shared__ double cs[VIO_MAXW * 3 + 10], sn[VIO_MAXW * 3 + 10];
    __shared__ int pp[VIO_MAXW * 3 + 10], qq[VIO_MAXW * 3 + 10];
    __shared__ double A15[225], V15[225], Pinv[225];
    __shared__ int newpresent[VIO_MAXW + 3];
    const bool second_new = PART == 2 ? msnap->second_new != 0 : be.marginalization_flag != 0;
    if (PART != 2 && second_new && !(be.has_prior && be.prior_present[W - 1])) return;
    // marg_exact: MarginalizationInfo::marginalize followed literally (marginalization_factor.cpp:281-315) -- the full m x m block of
    // pose 0, speed-bias 0 AND the landmarks that start in frame 0 goes through one truncated eigen-decomposition, and the new prior is
    // rebuilt from the truncated factors of the reduced system.  A parity instrument (one workgroup), not the hot path.
    const bool exact = EXACT && cfg.marg_exact == 1 && c.margE != nullptr;
    // marg_exact = 2 (round 5): the literal algorithm with its first eigen-decomposition replaced by a CERTIFIED inverse.  A_mm^+ of the
    // reference (:281-283) equals A_mm^-1 whenever no eigenvalue of A_mm is at or below the 1e-8 cut; this mode eliminates the marginalised
    // block exactly like the default one (landmarks analytically, the 15 x 15 / 6 x 6 rest by a Cholesky inverse) and PROVES per frame that
    // nothing could have been truncated: lambda_min(A_mm) >= 1 / |A_mm^-1|_F, bounded from the blocks of the inverse (below).  The second
    // half -- the factorisation of the new prior with its 1e-8 truncation, which does drop directions routinely -- is the literal one
    // (marg_literal_prior).  Frames whose certificate fails are counted (BeSeq::dbg[12]) and take the same route.
    const bool lit2 = EXACT && cfg.marg_exact == 2;
    int F0x = 0;   // landmarks in the marginalised block (exact mode)
    int F0k = 0;   // landmarks eliminated analytically (the other modes)
    PH_INIT;
    const long long tk0 = VIO_CLOCK();
    // vector2double
    constexpr int NX = (int)(offsetof(Params, relo) / sizeof(double));   // what a MargSnap carries of X
    if constexpr (PART == 2) {
        for (int k = t; k < NX; k += nt) ((double *)&X)[k] = ((const double *)&msnap->X)[k];
    } else {
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
    }
    }
    if (t < W + 3) newpresent[t] = 0;
    __syncthreads();
    if (PART != 2 && t <= W) for (int k = 0; k < 7; k++) be.para_Pose[t][k] = X.pose[t * 7 + k];   // (the marginalisation's vector2double: see solve_epilogue)
    if constexpr (PART == 1) {
        // the hand-over record: the slots of X the window fills (the rest of the LDS image is never read: every loop over frames stops at W)
        for (int k = t; k < NX; k += nt) {
            const bool set = k < (W + 1) * 7 || (k >= (VIO_MAXW + 1) * 7 && k < (VIO_MAXW + 1) * 7 + (W + 1) * 9) || k >= (VIO_MAXW + 1) * 16;
            ((double *)&msnap->X)[k] = set ? ((const double *)&X)[k] : 0.0;
        }
        if (t == 0) {
            msnap->second_new = second_new ? 1 : 0; msnap->pre1 = be.pre_idx[1]; msnap->F0c = 0;
            for (int k = 0; k < 3; k++) msnap->g[k] = be.g[k];
            msnap->active = 1;
        }
    }
    // reduced system over q = [m-block (md) | kept block (n)]
    const int md = second_new ? 6 : 15;
    const int mq = md + n;
    // (LDSA: behind the overlay region, laid out for md = 15; the overlay itself holds Jw, then G_j, then T1 / A_mr, then the tiles of c0)
    double *const ovl = (double *)smem_marg;
    double *const Ares = (double *)(smem_marg + marg_overlay_bytes(n, W, true));
    double *A = LDSA ? Ares : c.margA, *b = LDSA ? Ares + (size_t)(n + 15) * (n + 15) : c.margB;
    double *Gj = LDSA ? ovl : c.pairblk;   // frame blocks, W x 210
    // index maps (canonical kept layout: pose slots 0..W-1, sb, ex, td)
    const int rS = md + 6 * W, rE = md + 6 * W + 9, rT = md + 6 * W + 15;
    if constexpr (PART != 1) {
    for (int i = t; i < mq * mq; i += nt) A[i] = 0;
    for (int i = t; i < mq; i += nt) b[i] = 0;
    __syncthreads();
    // prior
    if (be.has_prior) {
        prior_dx(c, X, sdx);
        // (round 6: the loops of this kernel that walked HBM one dependent load at a time -- a load behind a store the compiler must assume to
        //  alias, or a runtime-bound loop with the load inside -- now issue their loads in batches; same terms in the same order, same bits.
        //  At W = 20 the kernel took 1.1 ms, none of its phases more than 0.2.)
        for (int i = t; i < n; i += nt) {  // prior gradient at the current state: b + A dx (A is stored exactly symmetric: read by columns, coalesced)
            double sacc = c.prior_r[i];
            for (int j0 = 0; j0 < n; j0 += 32) {
                double hv[32];
#pragma unroll
                for (int u = 0; u < 32; u++) hv[u] = c.prior_H[(size_t)min(j0 + u, n - 1) * n + i];
#pragma unroll
                for (int u = 0; u < 32; u++) if (j0 + u < n) sacc += hv[u] * sdx[j0 + u];
            }
            srp[i] = sacc;
        }
        __syncthreads();
        auto pmap = [&](int a) -> int {
            if (a < 6 * W) {
                int k = a / 6, d = a - 6 * k;
                if (second_new) return k == W - 1 ? d : md + 6 * k + d;
                return k == 0 ? d : md + 6 * (k - 1) + d;
            }
            if (a < 6 * W + 9) return second_new ? rS + (a - 6 * W) : 6 + (a - 6 * W);
            if (a < 6 * W + 15) return rE + (a - 6 * W - 9);
            return rT;
        };
        for (int w0 = t; w0 < n * n; w0 += 8 * nt) {  // J^T J of the prior is kept next to J (prior_H, written when the prior was built); A is still zero here
            double pv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) pv[u] = c.prior_H[min(w0 + u * nt, n * n - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int w = w0 + u * nt;
                if (w < n * n) { const int a = w / n, bb = w - a * n; A[pmap(a) * mq + pmap(bb)] = 0.0 + pv[u]; }
            }
        }
        for (int a = t; a < n; a += nt) b[pmap(a)] += srp[a];
        if (t < W + 3) {
            const int pres = be.prior_present[t];
            if (t > W) { if (pres) newpresent[t] = 1; }
            else if (second_new) { if (t < W - 1 || t == W) newpresent[t] = pres; }
            else if (t >= 1 && t < W && pres) newpresent[t - 1] = 1;
        }
        __syncthreads();
    }
    }
    PH(16);
    if (!second_new) {
        if constexpr (PART != 1) {
        // IMU factor (0,1)
        PreInt &p1 = c.pre[PART == 2 ? msnap->pre1 : be.pre_idx[1]];
        const v3 grav = PART == 2 ? ld3(msnap->g) : ld3(be.g);
        if (cfg.use_imu && bf::imu_marg_uses(p1)) {
            double *Jw = Gj;                // 15x30 whitened (the frame blocks' place, before they exist)
            double *raw = c.imu_raw;        // 15x31
            // five work types (whitened residual + four Jacobian column groups), each on its own wavefront, like evaluate()
            if ((t & 63) == 0) for (int part = t >> 6; part < 5; part += nt >> 6) {
                double unused = 0;   // (the marginalisation has no use for the cost)
                bf::imu_work_item(p1, false, grav, &X.pose[0], &X.sb[0], &X.pose[7], &X.sb[9], part, true, raw, unused);
            }
            __syncthreads();
            for (int w = t; w < 450; w += nt) {
                int r = w / 30, col = w - r * 30;
                double sacc = 0;
                for (int k = 0; k <= r; k++) sacc += p1.sqrt_info[r * 15 + k] * raw[k * 31 + col];
                Jw[w] = sacc;
            }
            __syncthreads();
            for (int w = t; w < 930; w += nt) {
                int a = w / 31, bb = w - a * 31;
                int ia = a < 15 ? a : (a < 21 ? md + (a - 15) : rS + (a - 21));
                double sacc = 0;
                if (bb < 30) {
                    int ib = bb < 15 ? bb : (bb < 21 ? md + (bb - 15) : rS + (bb - 21));
                    for (int k = 0; k < 15; k++) sacc += Jw[k * 30 + a] * Jw[k * 30 + bb];
                    A[ia * mq + ib] += sacc;
                } else {
                    for (int k = 0; k < 15; k++) sacc += Jw[k * 30 + a] * raw[k * 31 + 30];
                    b[ia] += sacc;
                }
            }
            if (t == 0) { newpresent[0] = 1; newpresent[W] = 1; }
            __syncthreads();
        }
        }
        PH(17);
        // projection factors of landmarks first observed in frame 0; each landmark is eliminated on the fly:
        // contribution = J_q^T J_q - c c^T / d  with c = J_q^T J_l, d = J_l^T J_l (pseudo-inverse: dropped if d <= eps)
        // (split: the list and each entry's observation count live in the marginalisation's own array -- pair_list and the landmark tables are
        //  the next frame's by the time PART 2 reads them)
        int *const list0 = PART ? mlist : c.pair_list;
        const int *const lno0 = PART ? mlist + c.NL : nullptr;
        auto lm_no0 = [&](int li) -> int { if constexpr (PART == 2) return lno0[li]; else return c.lm_nobs[list0[li]]; };
        const int per = W;  // max residuals per landmark
        int F0c;
        if constexpr (PART != 2) {
        int nlm = be.n_lm;
        int *flag = c.lm_tmp, *offs = c.res_k;
        for (int k = t; k < nlm; k += nt) { int slot = c.lm_order[k]; flag[k] = (in_problem(c, slot) && c.lm_start[slot] == 0) ? 1 : 0; }
        __syncthreads();
        int F0 = block_scan_flags(flag, nlm, offs, scratch);
        for (int k = t; k < nlm; k += nt) if (flag[k]) list0[offs[k]] = c.lm_order[k];
        __syncthreads();
        // per landmark: evaluate residuals with loss correction, store J (2x20) r (2) per residual into c.res (cap checked)
        F0c = min(F0, c.nres_cap / per);
        } else F0c = msnap->F0c;
        if (exact) { F0c = min(F0c, min(C.MX - 15, 480)); F0x = F0c; }
        F0k = F0c;
        if constexpr (PART != 2) {
        // frame-pair form like the solver (be_factors.h eval_projection_pair): the geometry of the pairs (0, k) once, in LDS
        __shared__ double mgeo[(VIO_MAXW + 1) * 32 + 16];
        stage_pair_geo(X, mgeo, W, nt, [](const int p, int &i, int &j) { i = 0; j = p + 1; return true; });
        for (int w = t; w < F0c * per; w += nt) {
            int li = w / per, k = w - li * per + 1;
            int slot = list0[li];
            double *out = c.res + (size_t)w * 42;
            if (k >= c.lm_nobs[slot]) { out[40] = 0; out[41] = 0; for (int q = 0; q < 40; q++) out[q] = 0; continue; }
            // CauchyLoss(1.0): rho'' < 0, so Ceres' corrector reduces to the scaling sqrt(rho') of residual and Jacobian (corrector.cc)
            double rr[2], wgt = 1.0;
            const double inv_dep = 1.0 / c.lm_depth[slot];
            const bf::PairGeo &g = *(const bf::PairGeo *)(mgeo + (size_t)(k - 1) * 32);
            bf::eval_projection_pair(cfg, g, mgeo + (size_t)W * 32, X.ex, inv_dep, X.td, c.K->tr, obs_ptr(c, slot, 0), obs_ptr(c, slot, k), cfg.estimate_td != 0, rr, out,
                                     true, &wgt);
            out[40] = wgt * rr[0];
            out[41] = wgt * rr[1];
        }
        __syncthreads();
        }
        PH(18);
        if constexpr (PART == 1) {
            for (int li = t; li < F0c; li += nt) mlist[c.NL + li] = c.lm_nobs[list0[li]];
            if (t == 0) msnap->F0c = F0c;
        }
        if constexpr (PART != 1) {
        // column map of a residual's 19 non-landmark columns into q: pose0 -> 0..5, pose_k -> md+6(k-1), ex, td
        // accumulate A_qq and b_q: thread per (a,b) over the union index set is irregular; use per-landmark dense rows:
        // c_l (mq), d_l, b_l, then A -= c c^T/d after adding the plain J^T J per residual.
        double *Cl = c.Hpl;  // F0c x LW' rows (reuse): needs mq + 2 <= LW  (mq = 15 + 6W + 16 = 6W+31 <= 15W+22 = P)
        const int ldc = c.LW;
        for (int w = t; w < F0c * ldc; w += nt) Cl[w] = 0;
        __syncthreads();
        // per landmark: c_l = J_q^T J_l over its residuals, d_l = J_l^T J_l, b_l = J_l^T r.  Sixteen lanes per landmark, lane = residual
        // (frame k = lane + 1): the columns of the lane's own frame are written directly, the columns every residual shares
        // (oldest pose, extrinsic, td) and d_l / b_l are reduced over the sixteen lanes.
        {
            const int grp = t >> 4, gln = t & 15, ngrp = nt >> 4;
            for (int li0 = 0; li0 < F0c; li0 += ngrp) {
                const int li = li0 + grp;
                const bool act = li < F0c;
                const int no = act ? lm_no0(li) : 0;
                double cm[13], dsum = 0, bsum = 0;
#pragma unroll
                for (int q = 0; q < 13; q++) cm[q] = 0;
                for (int k = gln + 1; k < no; k += 16) {
                    const double *Jg = c.res + (size_t)(li * per + k - 1) * 42;
                    double Jr[42];   // the whole record first: the stores to Cl below would otherwise sit between its loads
#pragma unroll
                    for (int q = 0; q < 42; q++) Jr[q] = Jg[q];
                    const double jl0 = Jr[19], jl1 = Jr[39];
#pragma unroll
                    for (int q = 0; q < 6; q++) {
                        cm[q] += Jr[q] * jl0 + Jr[20 + q] * jl1;
                        cm[6 + q] += Jr[12 + q] * jl0 + Jr[32 + q] * jl1;
                        Cl[(size_t)li * ldc + md + 6 * (k - 1) + q] = Jr[6 + q] * jl0 + Jr[26 + q] * jl1;
                    }
                    if (cfg.estimate_td) cm[12] += Jr[18] * jl0 + Jr[38] * jl1;
                    dsum += jl0 * jl0 + jl1 * jl1;
                    bsum += jl0 * Jr[40] + jl1 * Jr[41];
                }
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
#pragma unroll
                    for (int q = 0; q < 13; q++) cm[q] += __shfl_xor(cm[q], off, 16);
                    dsum += __shfl_xor(dsum, off, 16);
                    bsum += __shfl_xor(bsum, off, 16);
                }
                if (act && gln == 0) {
#pragma unroll
                    for (int q = 0; q < 6; q++) { Cl[(size_t)li * ldc + q] = cm[q]; Cl[(size_t)li * ldc + rE + q] = cm[6 + q]; }
                    if (cfg.estimate_td) Cl[(size_t)li * ldc + rT] = cm[12];
                    c.Hll[li] = dsum;
                    c.gl[li] = bsum;
                }
            }
        }
        __syncthreads();
        PH(19);
        // frame blocks G_j = sum over the residuals observing frame j of [J19 r]^T [J19 r] (packed symmetric 20x20) on the FP64
        // matrix cores: one wavefront per frame, K = 2 rows per landmark (rows of landmarks that do not see frame j are zero)
        {
            const int lane = t & 63, wave = t >> 6, nw = nt >> 6, li = lane & 15, lk = lane >> 4;
            for (int j = 1 + wave; j <= W; j += nw) {
                v4f64 a00 = {0, 0, 0, 0}, a10 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
                const int K = 2 * F0c;
                for (int k0 = 0; k0 < K; k0 += 64) {   // four 16-row trips' loads in flight at once, the matrix-core steps in the order of the one-trip loop
                    double x0[16], x1[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        int kk = k0 + 4 * u + lk;
                        bool valid = kk < K;
                        int lm = min(kk, K - 1) >> 1, sub = kk & 1;
                        const double *Jr = c.res + (size_t)(lm * per + j - 1) * 42;
                        double v0 = Jr[sub * 20 + li];
                        double v1 = Jr[li < 3 ? sub * 20 + 16 + li : 40 + sub];
                        x0[u] = valid ? v0 : 0.0;
                        x1[u] = (valid && li < 4) ? v1 : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        if (k0 + 16 * (u >> 2) >= K) break;
                        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], x0[u], a00, 0, 0, 0);
                        a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], x0[u], a10, 0, 0, 0);
                        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], x1[u], a11, 0, 0, 0);
                    }
                }
                double *out = Gj + (size_t)(j - 1) * 210;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int row = lk + 4 * r, col = li;
                    if (col <= row) out[sym_idx(col, row)] = a00[r];
                    if (row < 4) out[sym_idx(col, 16 + row)] = a10[r];
                    if (row < 4 && col < 4 && col <= row) out[sym_idx(16 + col, 16 + row)] = a11[r];
                }
            }
        }
        if (!exact) for (int li = t; li < F0c; li += nt) { double d = c.Hll[li]; c.Hll[li] = d > eps ? 1.0 / d : 0.0; }  // pseudo-inverse of the diagonal block
        __syncthreads();
        PH(24);
        // A_qq += sum_j G_j (scattered) - C^T D^+ C ; b_q likewise.  Per q-column (and the right-hand side, index mq): the frame whose
        // residuals carry it (0 = every residual: oldest pose, extrinsic, td, rhs; -1 = none) and its local column in a residual record
        __shared__ signed char qfr[6 * VIO_MAXW + 40], qlc[6 * VIO_MAXW + 40];
        __shared__ double sub_part[4][6 * VIO_MAXW + 40];
        for (int a = t; a <= mq; a += nt) {
            int fr = -1, lc = 0;
            if (a == mq) { fr = 0; lc = 19; }
            else if (a < 6) { fr = 0; lc = a; }
            else if (a >= md && a < md + 6 * W) { fr = (a - md) / 6 + 1; lc = 6 + (a - md) % 6; }
            else if (a >= rE && a < rE + 6) { fr = 0; lc = 12 + (a - rE); }
            else if (a == rT && cfg.estimate_td) { fr = 0; lc = 18; }
            qfr[a] = (signed char)fr; qlc[a] = (signed char)lc;
        }
        // b_q -= C^T D^+ b_l: four interleaved partial sums per column, added in a fixed order
        for (int w = t; w < 4 * mq; w += nt) {
            const int ch = w / mq, a = w - ch * mq;
            double acc = 0;
            if (!exact) for (int li = ch; li < F0c; li += 4) acc += Cl[(size_t)li * ldc + a] * (c.gl[li] * c.Hll[li]);
            sub_part[ch][a] = acc;
        }
        __syncthreads();
        for (int w0 = t; w0 < mq * (mq + 1); w0 += 4 * nt) {   // four entries per thread and trip: their gathers and the entries of A they add to in flight together
            bool use[4], multi[4], rhs[4];
            int dst[4], row[4], sidx[4];
            double pv[4], av[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int w = min(w0 + u * nt, mq * (mq + 1) - 1);
                const int a = w / (mq + 1), bb = w - a * (mq + 1);
                const int fa = qfr[a], fb = qfr[bb];
                const int la = qlc[a], lb = qlc[bb];
                use[u] = w0 + u * nt < mq * (mq + 1) && fa >= 0 && fb >= 0 && !(fa > 0 && fb > 0 && fa != fb);
                multi[u] = use[u] && fa == 0 && fb == 0;
                rhs[u] = bb == mq; row[u] = a; dst[u] = a * mq + bb;
                sidx[u] = sym_idx(la, lb);
                const int f1 = fa > 0 ? fa : (fb > 0 ? fb : 1);
                pv[u] = use[u] ? Gj[(size_t)(f1 - 1) * 210 + sidx[u]] : 0.0;
                av[u] = use[u] ? (rhs[u] ? b[a] : A[dst[u]]) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (!use[u]) continue;
                double sacc = pv[u];
                if (multi[u]) {   // a column every residual carries against another such: one term per frame, all loads first
                    double fv[VIO_MAXW];
#pragma unroll
                    for (int j = 0; j < VIO_MAXW; j++) fv[j] = Gj[(size_t)min(j, W - 1) * 210 + sidx[u]];
                    sacc = 0;
#pragma unroll
                    for (int j = 0; j < VIO_MAXW; j++) if (j < W) sacc += fv[j];
                }
                if (!rhs[u]) A[dst[u]] = av[u] + sacc;
                else b[row[u]] = av[u] + (sacc - ((sub_part[0][row[u]] + sub_part[1][row[u]]) + (sub_part[2][row[u]] + sub_part[3][row[u]])));
            }
        }
        __syncthreads();
        PH(25);
        // A_qq -= C^T D^+ C : rank-F0c update on the FP64 matrix cores, lower 16x16 tiles mirrored into the upper triangle
        if (!exact) {
            const int lane = t & 63, wave = t >> 6, nw = nt >> 6, li = lane & 15, lk = lane >> 4;
            const int nbq = (mq + 15) >> 4, ntile = nbq * (nbq + 1) / 2;
            for (int tile = wave; tile < ntile; tile += nw) {
                int ti, tj;
                tri_decode(tile, ti, tj);
                v4f64 acc = {0, 0, 0, 0};
                const int ca = min(16 * ti + li, ldc - 1), cb = min(16 * tj + li, ldc - 1);
                for (int k0 = 0; k0 < F0c; k0 += 64) {   // (four trips' loads in flight, as above)
                    double xa[16], xb[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        int kk = k0 + 4 * u + lk;
                        bool valid = kk < F0c;
                        int kc = min(kk, F0c - 1);
                        double va = Cl[(size_t)kc * ldc + ca], vb = Cl[(size_t)kc * ldc + cb], dinv = c.Hll[kc];
                        xa[u] = valid ? -(va * dinv) : 0.0;
                        xb[u] = valid ? vb : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        if (k0 + 16 * (u >> 2) >= F0c) break;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u], xb[u], acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int row = 16 * ti + lk + 4 * r, col = 16 * tj + li;
                    if (row < mq && col < mq && (ti != tj || col <= row)) {
                        A[row * mq + col] += acc[r];
                        if (row != col) A[col * mq + row] += acc[r];
                    }
                }
            }
        }
        for (int li = t; li < F0c; li += nt) {   // every writer stores the same value
            int no = lm_no0(li);
            for (int k = 1; k < no; k++) newpresent[k - 1] = 1;
            if (no > 1) { newpresent[W + 1] = 1; if (cfg.estimate_td) newpresent[W + 2] = 1; }
        }
        __syncthreads();
        }
    }
    if constexpr (PART == 1) return;   // (the window slide follows: be_marg_pre_kernel)
    else {
    if (VIO_TIMERS && s == 0 && t == 0 && !second_new) B.timings[31] += 1.0f;
    PH(20);
    if (exact) marg_exact_finish(c, be, A, b, md, mq, n, c.Hpl, c.LW, F0x, second_new, sred);
    else {
    // ---- eliminate the m-block (md x md) with a truncated eigen-decomposition
    for (int w = t; w < md * md; w += nt) { int i = w / md, j = w - i * md; A15[w] = 0.5 * (A[i * mq + j] + A[j * mq + i]); }
    __syncthreads();
    // Pseudo-inverse with the eigenvalues <= 1e-8 dropped.  Fast path: when a Cholesky factorisation proves every eigenvalue above 1e-6
    // (lambda_min >= 1 / |A^-1|_F) nothing is dropped and the pseudo-inverse is the inverse, a few microseconds of one wavefront instead
    // of ~100 Jacobi rounds; otherwise the eigen-decomposition decides.  Kept identical to be_linalg.h marg_pinv15 (its harness and tests).
    __shared__ int pinv_direct;
    __shared__ double L15[225];
    if (t < 64) {
        const bool okc = spd_inverse_wave16(A15, md, 1e-6, L15, V15, Pinv);
        if (t == 0) pinv_direct = okc ? 1 : 0;
    }
    __syncthreads();
    if (!pinv_direct) {
        if (t < 64) jacobi_wave16(A15, V15, md, md, cs, sn, pp, qq);   // md <= 15: one wavefront, no workgroup barriers inside
        __syncthreads();
        for (int w = t; w < md * md; w += nt) {
            int i = w / md, j = w - i * md;
            double sacc = 0;
            for (int k = 0; k < md; k++) { double ev = A15[k * md + k]; if (ev > eps) sacc += V15[i * md + k] * V15[j * md + k] / ev; }
            Pinv[w] = sacc;
        }
        __syncthreads();
    }
    if (VIO_TIMERS && s == 0 && t == 0 && pinv_direct) B.timings[26] += 1.0f;
    PH(36);
    // T1 = A_rm A_mm^+ (n x md) and the block A_mr (md x n) staged in LDS (the tile region, free until the constant term is formed): the
    // n^2 entries of A_r = A_rr - T1 A_mr read each of them n times
    double *T1 = (double *)smem_marg, *Amr = T1 + (size_t)n * md;
    for (int w = t; w < n * md; w += nt) {
        int i = w / md, j = w - i * md;
        double sacc = 0;
        for (int k = 0; k < md; k++) sacc += A[(md + i) * mq + k] * Pinv[k * md + j];
        T1[w] = sacc;
        const int k2 = w / n, j2 = w - k2 * n;      // the same index range covers A_mr (md x n)
        Amr[w] = A[k2 * mq + md + j2];
    }
    __syncthreads();
    PH(37);
    // A_r (n x n): c.margV, or (LDSA) in place in the kept block of A -- each entry needs its own entry of A and the staged T1 / A_mr only
    const int lda = LDSA ? mq : n;
    double *Ar = LDSA ? A + (size_t)md * mq + md : c.margV;
    double *br = LDSA ? Ares + (size_t)(n + 15) * (n + 16) : c.vec;   // n
    for (int w0 = t; w0 < n * n; w0 += 8 * nt) {
        double av[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int w = min(w0 + u * nt, n * n - 1), i = w / n, j = w - i * n; av[u] = A[(md + i) * mq + md + j]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int w = w0 + u * nt;
            if (w >= n * n) break;
            const int i = w / n, j = w - i * n;
            double tt = av[u];
            for (int k = 0; k < md; k++) tt -= T1[i * md + k] * Amr[k * n + j];
            Ar[i * lda + j] = tt;
        }
    }
    for (int i = t; i < n; i += nt) {
        double sacc = b[md + i];
        for (int k = 0; k < md; k++) sacc -= T1[i * md + k] * b[k];
        br[i] = sacc;
    }
    __syncthreads();
    PH(21);
    if (lit2) {
        const bool certified = marg_certificate(Pinv, md, pinv_direct, second_new, c.Hpl, c.LW, c.Hll, F0k, sred, nullptr);
        if (t == 0) {
            be.dbg[11] = certified ? 1 : 0;
            if (!certified) be.dbg[12] += 1;
        }
        __syncthreads();
        marg_literal_prior(c, be, Ar, br, n, c.margW, sred);
        if (t == 0) { be.dbg[0] = 0; be.dbg[2] = second_new ? 1 : 0; be.dbg[4] = md; }
    } else {
    // ---- the new prior, kept as the quadratic form the solver consumes: A = sym(A_r), b = b_r, c0 = b^T A^+ b.
    // The reference factors A = V S V^T, drops eigenvalues <= 1e-8 and stores J = S^1/2 V^T, r = S^-1/2 V^T b
    // (marginalization_factor.cpp:293-315); J^T J, J^T r and |r|^2 are all the solver and the next marginalisation ever use, and
    // they equal (A, b, c0) up to the dropped directions: measured on the canonical workload b has a 1e-12 relative component
    // there, A changes by < 1e-8 absolute (1e-16 relative) and the weakly observed directions contribute < 1e-5 of c0
    // (DESIGN.md deviation 13).  The factored form is produced on demand by be_prior_factor_kernel (vio_get_prior).
    for (int w0 = t; w0 < n * n; w0 += 8 * nt) {
        double x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int w = min(w0 + u * nt, n * n - 1), i = w / n, j = w - i * n; x[u] = Ar[i * lda + j]; y[u] = Ar[j * lda + i]; }
#pragma unroll
        for (int u = 0; u < 8; u++) if (w0 + u * nt < n * n) c.prior_H[w0 + u * nt] = 0.5 * (x[u] + y[u]);
    }
    for (int i = t; i < n; i += nt) c.prior_r[i] = br[i];
    PH(38);
    {
        // c0 = |L^-1 b|^2 with L L^T = A + delta I on 16x16 LDS tiles (delta lifts the gauge directions off the round-off floor)
        __shared__ __attribute__((aligned(16))) double cq_x[EIG_LD + 16];   // read and written in 16-byte pairs by chol_tiles
        __shared__ double cq_dinv[EIG_LD + 16];
        __shared__ int cq_flag;
        const int nbq = (n + 15) >> 4;
        double *T = (double *)smem_marg;
        double dmax = 0;
        for (int i = t; i < n; i += nt) dmax = fmax(dmax, fabs(Ar[i * lda + i]));
        dmax = block_max(dmax, sred);
        const double delta = 64.0 * 2.220446049250313e-16 * (double)n * dmax;
        const int ntl = nbq * (nbq + 1) / 2 * 256;
        for (int w0 = t; w0 < ntl; w0 += 4 * nt) {
            double x[4], y[4];
            int ii[4], jj[4], dd[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int w = min(w0 + u * nt, ntl - 1);
                int tile = w >> 8, e = w & 255, r = e >> 4, cc = e & 15, ti, tj;
                tri_decode(tile, ti, tj);
                const int i = 16 * ti + r, j = 16 * tj + cc, ic = min(i, n - 1), jc = min(j, n - 1);
                ii[u] = i; jj[u] = j; dd[u] = tl_idx(ti, tj, r, cc);
                x[u] = Ar[ic * lda + jc]; y[u] = Ar[jc * lda + ic];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (w0 + u * nt >= ntl) break;
                const int i = ii[u], j = jj[u];
                T[dd[u]] = (i < n && j < n) ? 0.5 * (x[u] + y[u]) + (i == j ? delta : 0.0) : (i == j ? 1.0 : 0.0);
            }
        }
        for (int i = t; i < 16 * nbq; i += nt) cq_x[i] = i < n ? br[i] : 0.0;
        __syncthreads();
        PH(39);
        double c0 = 0;
        if (dmax > 0 && chol_tiles(T, nbq, &cq_flag, cq_dinv, nullptr, cq_x)) {   // c0 needs the forward substitution only
            double acc = 0;
            for (int i = t; i < n; i += nt) acc += cq_x[i] * cq_x[i];
            c0 = block_sum(acc, sred);
            if (!isfinite(c0)) c0 = 0;
        }
        __syncthreads();
        if (t == 0) { be.prior_c0 = c0; be.dbg[0] = 0; be.dbg[2] = second_new ? 1 : 0; }
    }
    }
    }
    PH(22);
    // keep_block_data in the shifted (canonical) layout
    if (t < W) {
        int src = second_new ? (t == W - 1 ? W : t) : t + 1;
        for (int d = 0; d < 7; d++) c.prior_x0[t * 7 + d] = X.pose[src * 7 + d];
    }
    if (t == W) for (int d = 0; d < 9; d++) c.prior_x0[W * 7 + d] = X.sb[(second_new ? 0 : 1) * 9 + d];
    if (t == W + 1) { for (int d = 0; d < 7; d++) c.prior_x0[W * 7 + 9 + d] = X.ex[d]; c.prior_x0[W * 7 + 16] = X.td; }
    __syncthreads();
    if (t < W + 3) be.prior_present[t] = newpresent[t];
    if (t == 0) { be.has_prior = 1; be.dbg[3] = (int)(VIO_CLOCK() - tk0); }
    if (PART == 2 && t == 0) msnap->frames++;
    PH(23);
    }
}

// Estimator::setReloFrame (estimator.cpp:1728-1747) for sequence seq; the match points are already in B.relo_mp.  par = stamp, index,
// n, relo_t(3), relo_r(9).  relo_Pose is copied from para_Pose[i] AS THE LAST optimization() LEFT IT, like upstream: after a MARGIN_OLD
// slide that array still holds the pre-slide window (the copy is then the pose of the frame one slot older), an upstream quirk that the
// first iterations of the relocalisation solve absorb.
__global__ void be_set_relo_kernel(Batch B, int seq, const double *par) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    BeSeq &be = B.be[seq];
    const int W = B.cfg->W;
    be.relo_stamp = par[0];
    be.relo_index = (int)par[1];
    be.relo_nmatch = (int)par[2];
    for (int k = 0; k < 3; k++) be.prev_relo_t[k] = par[3 + k];
    for (int k = 0; k < 9; k++) be.prev_relo_r[k] = par[6 + k];
    for (int i = 0; i < W; i++)
        if (be.relo_stamp == be.Headers[i]) {
            be.relo_local = i;
            be.relo_info = 1;
            for (int j = 0; j < 7; j++) be.relo_Pose[j] = be.para_Pose[i][j];
            // before the first optimization() nothing has written para_Pose (upstream copies indeterminate memory there): the state holds
            // zeros, and the copy is the identity pose, as in the oracle
            if (be.relo_Pose[3] == 0 && be.relo_Pose[4] == 0 && be.relo_Pose[5] == 0 && be.relo_Pose[6] == 0) be.relo_Pose[6] = 1.0;
        }
}

// ====================================================================================================== prior factorisation
// linearized_jacobians / linearized_residuals of the current prior (marginalization_factor.cpp:293-315), on demand: eigen-
// decomposition of prior_H with the 1e-8 cut-off, J = S^1/2 V^T -> prior_J, r = S^-1/2 V^T b -> prior_rf.
__global__ __launch_bounds__(512) void be_prior_factor_kernel(Batch B, int seq) {
    const int s = seq, t = threadIdx.x, nt = blockDim.x;
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_marg[];
    Ctx c = make_ctx(B, s);
    BeSeq &be = *c.be;
    if (!be.has_prior) return;
    const int n = c.NPR;
    const double eps = 1e-8;
    const double *br = c.prior_r;
    const long long tj0 = VIO_CLOCK();
    // symmetrised A_r and its eigenvectors live in LDS when they fit (n <= 96), else in HBM scratch
    const bool in_lds = n <= 96;
    const int ldj = in_lds ? (n | 1) : n;  // odd leading dimension: conflict-free 64-bit LDS column access
    double *As = in_lds ? (double *)smem_marg : c.margA;
    double *Vv = in_lds ? (double *)smem_marg + n * ldj : c.margW + (size_t)n * 16;
    for (int w = t; w < n * n; w += nt) { int i = w / n, j = w - i * n; As[i * ldj + j] = c.prior_H[w]; }
    __syncthreads();
    __shared__ double ev_d[6 * VIO_MAXW + 16], ev_e[6 * VIO_MAXW + 16], ev_g[6 * VIO_MAXW + 16];
    __shared__ double ev_part[8 * EIG_LD];
    // two call sites so that the eigen-solver is specialised for the address space of the matrix (ds_* for LDS, global_* for HBM)
    // instead of falling back to flat loads on a pointer that could be either
    if (in_lds) {
        double *Al = (double *)smem_marg;
        if ((nt >> 6) <= 8) sym_eig_tridiag_mt(Al, n, ldj, ev_d, ev_e, ev_g, ev_part);
        else sym_eig_tridiag(Al, n, ldj, ev_d, ev_e, ev_g, sred);
        if (t == 0) be.dbg[5] = (int)(VIO_CLOCK() - tj0);
        tridiag_ql_wave(Al, n, ldj, ev_d, ev_e);
    } else {
        double *Ag = c.margA;
        if ((nt >> 6) <= 8) sym_eig_tridiag_mt(Ag, n, ldj, ev_d, ev_e, ev_g, ev_part);
        else sym_eig_tridiag(Ag, n, ldj, ev_d, ev_e, ev_g, sred);
        if (t == 0) be.dbg[5] = (int)(VIO_CLOCK() - tj0);
        tridiag_ql_wave<3>(Ag, n, ldj, ev_d, ev_e);   // (n = 136 at W = 20: three rows per lane)
    }
    if (t == 0) be.dbg[6] = (int)(VIO_CLOCK() - tj0);
    Vv = As;  // eigenvectors overwrite the matrix
    if (t == 0) be.dbg[1] = (int)(VIO_CLOCK() - tj0);
    // linearized_jacobians = sqrt(S) V^T ; linearized_residuals = S^-1/2 V^T b
    for (int w = t; w < n * n; w += nt) {
        int k = w / n, i = w - k * n;
        double wv = ev_d[k];
        double S = wv > eps ? wv : 0.0;
        c.prior_J[w] = sqrt(S) * Vv[i * ldj + k];
    }
    for (int k = t; k < n; k += nt) {
        double wv = ev_d[k];
        double Sinv = wv > eps ? 1.0 / wv : 0.0;
        double vb = 0;
        for (int i = 0; i < n; i++) vb += Vv[i * ldj + k] * br[i];
        c.prior_rf[k] = sqrt(Sinv) * vb;
    }
}

// ====================================================================================================== be_finish
template <bool LT> __device__ void finish_body(const Batch &B, int s, int *scratch, PreWork &pw, unsigned char *smem_marg) {   // smem_marg: the marginalisation's dynamic LDS, free again (>= PREINT_MANY_LDS_DOUBLES doubles)
    const int t = threadIdx.x, nt = blockDim.x;
    Ctx c = make_ctx(B, s);
    const DevCfg &C = *B.cfg;
    const vio_config &cfg = C.c;
    BeSeq &be = *c.be;
    const int W = c.W, W1 = W + 1;
    __shared__ int sh_i[4];
    double *od = B.odom + (size_t)s * 11;
    if (!be.processed || be.rebooted) return;
    PH_INIT;
    int nlm = be.n_lm;
    // LT: the order list, the start frame and observation count of its entries (by position), the flags and the offsets staged in the dynamic LDS
    // where the reduced system was (MARG_LM_TABLES arrays of NL integers); n_lm / n_free in registers.  The order list, the flags and the offsets go
    // back to HBM once (stage_back): entry for entry what the two compactions in HBM leave, the stale tails included.
    int *const tab = (int *)(smem_marg + marg_overlay_bytes(c.NPR, W, true));
    int *const flag = LT ? tab + 2 * c.NL : c.lm_pidx, *const offs = LT ? tab + 3 * c.NL : c.lm_aidx;  // (HBM: free after the solve)
    int *const ord = LT ? tab : c.lm_order, *const otmp = tab + c.NL, *const lst = tab + 4 * c.NL, *const lno = tab + 5 * c.NL;
    const int nlm0 = nlm;
    int nfree = be.n_free;
    if (LT) for (int k = t; k < nlm; k += nt) { const int slot = c.lm_order[k]; ord[k] = slot; lst[k] = c.lm_start[slot]; lno[k] = c.lm_nobs[slot]; }
    auto lm_st = [&](int k, int slot) -> int { return LT ? lst[k] : c.lm_start[slot]; };
    auto lm_no = [&](int k, int slot) -> int { return LT ? lno[k] : c.lm_nobs[slot]; };
    auto compact = [&]() { if (LT) lm_compact_staged(c, ord, otmp, flag, offs, scratch, nlm, nfree); else lm_compact(c, flag, offs, scratch); };
    auto stage_back = [&]() {
        if (!LT) return;
        for (int k = t; k < nlm0; k += nt) { c.lm_order[k] = ord[k]; c.lm_pidx[k] = flag[k]; c.lm_aidx[k] = offs[k]; }
        if (t == 0) { be.n_lm = nlm; be.n_free = nfree; }
    };
    const int fc = be.frame_count;
    const int sflag0 = be.solver_flag;
    __syncthreads();
    // dynamic initialisation (static_init: 0, estimator.cpp:230-259): while INITIAL the frame counter just advances; with a full
    // window and no (successful) attempt the window slides with INITIAL semantics (removeBack, no depth transfer).  A static-initialisation
    // sequence whose full window is held by the extrinsic calibration (estimate_extrinsic = 2) slides the same way (DESIGN.md deviation 16;
    // upstream it neither initialises nor slides, estimator.cpp:262-316)
    const bool dyn_initial = sflag0 == 0 && (cfg.dynamic_init || (fc == W && !be.do_solve && be.ex_pending));
    if (dyn_initial) {
        if (fc < W) {
            if (t == 0) be.frame_count = fc + 1;
            return;
        }
    } else if (sflag0 == 0) {
        if (fc == W && be.do_solve) {
            if (t == 0) be.solver_flag = 1;
            __syncthreads();
        } else {
            // frame_count < WINDOW_SIZE: copy the state forward (estimator.cpp:306-315)
            if (t == 0 && fc < W) {
                int n = fc + 1;
                for (int k = 0; k < 3; k++) { be.Ps[n][k] = be.Ps[fc][k]; be.Vs[n][k] = be.Vs[fc][k]; be.Bas[n][k] = be.Bas[fc][k]; be.Bgs[n][k] = be.Bgs[fc][k]; }
                for (int k = 0; k < 9; k++) be.Rs[n][k] = be.Rs[fc][k];
                be.frame_count = n;
            }
            return;
        }
    } else if (!be.init_frame) {
        // movingConsistencyCheck (estimator.cpp:1965-2009); not on the frame that completed the dynamic initialisation (:243-251)
        m3 ric = ldm(be.ric);
        v3 tic = ld3(be.tic);
        for (int k = t; k < nlm; k += nt) {
            int slot = ord[k];
            const int imu_i = lm_st(k, slot), no = lm_no(k, slot);
            if (!(no >= 2 && imu_i < W - 2)) continue;
            double depth = c.lm_depth[slot];
            if (depth < 0) continue;
            const double *oi = obs_ptr(c, slot, imu_i);
            v3 pts_i = mk(oi[0], oi[1], oi[2]);
            double err = 0, err3 = 0;
            int cnt = 0;
            for (int q = 1; q < no; q++) {
                int imu_j = imu_i + q;
                const double *oj = obs_ptr(c, slot, imu_j);
                v3 pts_j = mk(oj[0], oj[1], oj[2]);
                v3 pts_w = add(mul(ldm(be.Rs[imu_i]), add(mul(ric, scl(depth, pts_i)), tic)), ld3(be.Ps[imu_i]));
                v3 pts_cj = mul(tr(ric), sub(mul(tr(ldm(be.Rs[imu_j])), sub(pts_w, ld3(be.Ps[imu_j]))), tic));
                double rx = pts_cj.x / pts_cj.z - pts_j.x, ry = pts_cj.y / pts_cj.z - pts_j.y;
                err += sqrt(rx * rx + ry * ry);
                err3 += nrm(sub(pts_cj, pts_j)) / depth;
                cnt++;
            }
            if (cnt > 0) c.lm_dyn[slot] = (cfg.focal_length * err / cnt > 10 || err3 / cnt > 2.0) ? 1 : 0;
        }
        __syncthreads();
        // failureDetection (estimator.cpp:1113-1159) ran at the end of be_solve (see there); a sequence that rebooted never gets here
    }
    PH(27);
    // ---- slideWindow (estimator.cpp:1580-1689)
    if (be.marginalization_flag == 0) {
        if (t == 0) {
            for (int k = 0; k < 9; k++) be.back_R0[k] = be.Rs[0][k];
            for (int k = 0; k < 3; k++) be.back_P0[k] = be.Ps[0][k];
            int first = be.pre_idx[0];
            for (int i = 0; i < W; i++) {
                be.Headers[i] = be.Headers[i + 1];
                for (int k = 0; k < 3; k++) { be.Ps[i][k] = be.Ps[i + 1][k]; be.Vs[i][k] = be.Vs[i + 1][k]; be.Bas[i][k] = be.Bas[i + 1][k]; be.Bgs[i][k] = be.Bgs[i + 1][k]; }
                for (int k = 0; k < 9; k++) be.Rs[i][k] = be.Rs[i + 1][k];
                be.pre_idx[i] = be.pre_idx[i + 1];
            }
            be.pre_idx[W] = first;
            // slot W keeps the newest state; its pre-integration restarts from acc_0 / gyr_0 (:1614-1630)
            bf::preint_init(c.pre[first], ld3(be.acc_0), ld3(be.gyr_0), ld3(be.Bas[W]), ld3(be.Bgs[W]));
        }
        __syncthreads();
        PH(28);
        // slideWindowOld -> removeBackShiftDepth (feature_manager.cpp:660-691); solver_flag is NON_LINEAR here
        m3 R0 = mul(ldm(be.back_R0), ldm(be.ric)), R1 = mul(ldm(be.Rs[0]), ldm(be.ric));
        v3 P0 = add(ld3(be.back_P0), mul(ldm(be.back_R0), ld3(be.tic))), P1 = add(ld3(be.Ps[0]), mul(ldm(be.Rs[0]), ld3(be.tic)));
        for (int k = t; k < nlm; k += nt) {
            int slot = ord[k];
            int keep = 1;
            const int st = lm_st(k, slot);
            if (st != 0) c.lm_start[slot] = st - 1;
            else {
                const double *o0 = obs_ptr(c, slot, 0);
                v3 uv_i = mk(o0[0], o0[1], o0[2]);
                int no = lm_no(k, slot) - 1;
                c.lm_nobs[slot] = no;
                if (dyn_initial) keep = no > 0;     // FeatureManager::removeBack (feature_manager.cpp:693-708): solver_flag == INITIAL
                else if (no < 2) keep = 0;
                else {
                    v3 pts_i = scl(c.lm_depth[slot], uv_i);
                    v3 w_pts_i = add(mul(R0, pts_i), P0);
                    v3 pts_j = mul(tr(R1), sub(w_pts_i, P1));
                    c.lm_depth[slot] = pts_j.z > 0 ? pts_j.z : cfg.init_depth;
                }
            }
            flag[k] = keep;
        }
        __syncthreads();
        if (t == 0) be.ring_base = (be.ring_base + 1) % W1;  // frame f becomes frame f-1 without moving observations
        __syncthreads();
        compact();
    } else {
        // MARGIN_SECOND_NEW: merge the IMU samples of frame W into W-1 (:1651-1687)
        PreInt &dst = c.pre[be.pre_idx[W - 1]];
        PreInt &src = c.pre[be.pre_idx[W]];
        if (t == 0) {
            be.Headers[W - 1] = be.Headers[W];
            for (int k = 0; k < 3; k++) { be.Ps[W - 1][k] = be.Ps[W][k]; be.Vs[W - 1][k] = be.Vs[W][k]; be.Bas[W - 1][k] = be.Bas[W][k]; be.Bgs[W - 1][k] = be.Bgs[W][k]; }
            for (int k = 0; k < 9; k++) be.Rs[W - 1][k] = be.Rs[W][k];
        }
        preint_load(dst, pw);
        PreintNoSide none;
        preint_propagate_many<false>(dst, pw, *c.K, src.n_buf, PreintArrays{src.dt_buf, src.acc_buf, src.gyr_buf}, none, true, (double *)smem_marg);
        preint_store(dst, pw);
        if (t == 0) bf::preint_init(src, ld3(be.acc_0), ld3(be.gyr_0), ld3(be.Bas[W]), ld3(be.Bgs[W]));
        __syncthreads();
        // slideWindowNew -> removeFront(frame_count) (feature_manager.cpp:710-730)
        for (int k = t; k < nlm; k += nt) {
            int slot = ord[k];
            int keep = 1;
            int st = lm_st(k, slot), no = lm_no(k, slot);
            if (st == W) {
                double *d = obs_ptr(c, slot, W - 1);
                const double *sr = obs_ptr(c, slot, W);
                for (int q = 0; q < VIO_OBS_D; q++) d[q] = sr[q];
                c.lm_start[slot] = st - 1;
            } else {
                int endf = st + no - 1;
                if (endf >= W - 1) {
                    if (endf == W) {
                        double *d = obs_ptr(c, slot, W - 1);
                        const double *sr = obs_ptr(c, slot, W);
                        for (int q = 0; q < VIO_OBS_D; q++) d[q] = sr[q];
                    }
                    c.lm_nobs[slot] = no - 1;
                    if (no - 1 == 0) keep = 0;
                }
            }
            flag[k] = keep;
        }
        __syncthreads();
        compact();
    }
    PH(29);
    if (dyn_initial) {   // still INITIAL: nothing to publish (the frame's flags still count)
        if (t == 0 && (be.overflow & ~VIO_OVF_DEVIATION)) be.overflow_frames++;
        stage_back();
        return;
    }
    // ---- removeFailures (feature_manager.cpp:225-233); not called on the STATIC initialisation frame (estimator.cpp:282-290)
    if (sflag0 == 1) {
        if (!LT) nlm = be.n_lm;
        for (int k = t; k < nlm; k += nt) flag[k] = c.lm_solve[ord[k]] == 2 ? 0 : 1;
        __syncthreads();
        compact();
    }
    stage_back();
    if (t == 0) {
        for (int k = 0; k < 9; k++) { be.last_R[k] = be.Rs[W][k]; be.last_R0[k] = be.Rs[0][k]; }
        for (int k = 0; k < 3; k++) { be.last_P[k] = be.Ps[W][k]; be.last_P0[k] = be.Ps[0][k]; }
        // CSV row of visualization.cpp:214-225
        quat q = R2q(ldm(be.Rs[W]));
        od[0] = be.Headers[W];
        od[1] = be.Ps[W][0]; od[2] = be.Ps[W][1]; od[3] = be.Ps[W][2];
        od[4] = q.w; od[5] = q.x; od[6] = q.y; od[7] = q.z;
        od[8] = be.Vs[W][0]; od[9] = be.Vs[W][1]; od[10] = be.Vs[W][2];
        int hc = B.odom_count[s];
        double *hrow = B.odom_hist + ((size_t)s * B.hist_cap + (hc % B.hist_cap)) * 11;  // ring: the getter un-rotates it
        for (int k = 0; k < 11; k++) hrow[k] = od[k];
        B.odom_count[s] = hc + 1;
        if (be.overflow & ~VIO_OVF_DEVIATION) be.overflow_frames++;   // (bit 512 reports a deviation, not lost capacity)
    }
    PH(30);
}

__global__ __launch_bounds__(1024) void be_solve_kernel(Batch B) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 1024 + 8];
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PreWork &pw = *(PreWork *)(smem + 16 * ((B.cfg->LW * 8 + 15) / 16));  // aliases the work region (used before it)
    solve_body(B, s, scratch, sred, smem, pw);
}
// the same body compiled for 512 threads: 256 VGPRs per lane instead of 128 (no scratch spills), half the waves
__global__ __launch_bounds__(512) void be_solve_kernel_512(Batch B) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 1024 + 8];
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PreWork &pw = *(PreWork *)(smem + 16 * ((B.cfg->LW * 8 + 15) / 16));
    solve_body(B, s, scratch, sred, smem, pw);
}
// marginalisation + window slide: 512 threads (measured: 2.9 ms against 3.5 ms with 256; the QL phase is one wavefront either way)
__global__ __launch_bounds__(512) void be_marg_kernel(Batch B) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 512 + 8];
    __shared__ double sred[64];
    __shared__ PreWork pw;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    marg_body<false, true>(B, s, scratch, sred, smem);
    __syncthreads();
    finish_body<true>(B, s, scratch, pw, smem);
}
// VIO_MARG_SPLIT (kernels.h): the same stage as two launches.  The first holds whatever touches window state the next frame's be_ingest / ps_setup
// share -- they follow it on the front-end stream, beside the second, which is the algebra and nothing else.
__global__ __launch_bounds__(512) void be_marg_pre_kernel(Batch B, MargSnap *snap, int *mlist) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 512 + 8];
    __shared__ double sred[64];
    __shared__ PreWork pw;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    marg_body<false, true, 1>(B, s, scratch, sred, smem, snap + s, mlist + (size_t)s * 2 * B.gNL);
    __syncthreads();
    finish_body<true>(B, s, scratch, pw, smem);
}
__global__ __launch_bounds__(512) void be_marg_alg_kernel(Batch B, MargSnap *snap, const int *mlist) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 512 + 8];
    __shared__ double sred[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    marg_body<false, true, 2>(B, s, scratch, sred, smem, snap + s, const_cast<int *>(mlist) + (size_t)s * 2 * B.gNL);
}
// the same stage with the reduced system, the frame blocks and the landmark tables in HBM scratch (rounds 1 - 6): windows whose system does not fit
// the workgroup's LDS (W = 12 and up) and VIO_MARG_LDS = 0
__global__ __launch_bounds__(512) void be_marg_hbm_kernel(Batch B) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 512 + 8];
    __shared__ double sred[64];
    __shared__ PreWork pw;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    marg_body<false, false>(B, s, scratch, sred, smem);
    __syncthreads();
    finish_body<false>(B, s, scratch, pw, smem);
}
// vio_config.marg_exact: the same stage with the marginalisation of marginalization_factor.cpp:281-315 followed literally (its own kernel so
// that the hot kernel's registers / LDS are untouched by the parity instrument)
__global__ __launch_bounds__(512) void be_marg_exact_kernel(Batch B) {
    const int s = blockIdx.x + B.s0;
    __shared__ int scratch[2 * 512 + 8];
    __shared__ double sred[64];
    __shared__ PreWork pw;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    marg_body<true, false>(B, s, scratch, sred, smem);
    __syncthreads();
    finish_body<false>(B, s, scratch, pw, smem);
}

// stage test of the literal marginalisation (kernels.h MargLiteralStage): marg_exact_finish / marg_literal_prior / marg_certificate as be_marg_exact_kernel
// calls them -- one workgroup of 256 or 512 threads, the dynamic LDS sized by the host with the production formulas, a Ctx that holds what they read
__global__ __launch_bounds__(512) void be_stage_marg_literal_kernel(MargLiteralStage a) {
    const int t = threadIdx.x, nt = blockDim.x;
    __shared__ double sred[64];
    __shared__ double Pinv[225];
    Ctx c = {};
    c.C = a.cfg; c.be = a.be; c.NPR = a.n; c.LW = a.ldc;
    c.Hpl = a.Cl; c.Hll = a.Hll; c.gl = a.gl; c.vec = a.vec;
    c.margE = a.margE; c.margV = a.margV; c.margW = a.margW;
    c.prior_J = a.prior_J; c.prior_H = a.prior_H; c.prior_r = a.prior_r; c.prior_rf = a.prior_rf;
    BeSeq &be = *c.be;
    if (a.part == 0) marg_exact_finish(c, be, a.A, a.b, a.md, a.md + a.n, a.n, c.Hpl, a.ldc, a.F0, a.second_new != 0, sred);
    else if (a.part == 1) marg_literal_prior(c, be, c.margV, c.vec, a.n, c.margW, sred);
    else {
        for (int w = t; w < a.md * a.md; w += nt) Pinv[w] = a.A[w];
        __syncthreads();
        const bool certified = marg_certificate(Pinv, a.md, a.pinv_direct, a.second_new != 0, c.Hpl, a.ldc, c.Hll, a.F0, sred, a.scal + 1);
        if (t == 0) a.info[0] = certified ? 1 : 0;
    }
    __syncthreads();
    if (t == 0) { a.scal[0] = be.prior_c0; a.info[1] = be.dbg[0]; a.info[2] = be.dbg[2]; a.info[3] = be.dbg[4]; }
}

// ====================================================================================================== stage tests
__global__ void be_stage_projection_kernel(vio_config cfg, const double *in /*pi7 pj7 ex7 inv_dep td oi9 oj9*/, int use_td, int form, double *r2, double *J46) {
    if (threadIdx.x != 0) return;
    // form 0: the frame-pair formulation the solver uses (evaluate()); form 1: bf::eval_projection, the per-residual form used by the
    // marginalisation and by outlier rejection
    double J[40], wgt;
    if (form == 0) {
        bf::PairGeo g;
        bf::pair_geo(in, in + 7, in + 14, g);
        double ricm[9];
        stm(ricm, q2R(mkq(in[14 + 6], in[14 + 3], in[14 + 4], in[14 + 5])));
        bf::eval_projection_pair(cfg, g, ricm, in + 14, in[21], in[22], cfg.tr, in + 23, in + 32, use_td != 0, r2, J, false, &wgt);
    } else
        bf::eval_projection(cfg, in, in + 7, in + 14, in[21], in[22], cfg.tr, in + 23, in + 32, use_td != 0, r2, J);
    for (int a = 0; a < 2; a++) {
        for (int d = 0; d < 6; d++) { J46[a * 7 + d] = J[a * 20 + d]; J46[14 + a * 7 + d] = J[a * 20 + 6 + d]; J46[28 + a * 7 + d] = J[a * 20 + 12 + d]; }
        J46[a * 7 + 6] = 0; J46[14 + a * 7 + 6] = 0; J46[28 + a * 7 + 6] = 0;
        J46[42 + a] = J[a * 20 + 19];
        J46[44 + a] = J[a * 20 + 18];
    }
}
// The IMU factor exactly as evaluate() + assemble() process it in the solver: raw residual whitened by thread 0, the four raw
// Jacobian column groups by imu_raw_jacobian_part, then [Jw r]^T [Jw r] on the matrix cores (imu_block_mfma).  One wavefront.
// G961: the 31 x 31 Gram matrix, row-major, columns = pose_i(6) speedbias_i(9) pose_j(6) speedbias_j(9) | r.
__global__ __launch_bounds__(64) void be_stage_imu_block_kernel(const PreInt *P, const double *par /*pi7 sbi9 pj7 sbj9*/, double g_norm, double *G961) {
    __shared__ double raw_l[472], M_l[232];
    const int lane = threadIdx.x;
    const PreInt &p = *P;
    v3 G = mk(0, 0, g_norm);
    if (lane == 0) {
        double raw[15];
        bf::imu_raw_residual(p, G, par, par + 7, par + 16, par + 23, raw);
        for (int r = 0; r < 15; r++) {
            double sacc = 0;
            for (int k = 0; k <= r; k++) sacc += p.sqrt_info[r * 15 + k] * raw[k];
            raw_l[r * 31 + 30] = sacc;
        }
    } else if (lane <= 4)
        bf::imu_raw_jacobian_part(p, G, par, par + 7, par + 16, par + 23, lane - 1, raw_l, 31);
    for (int q = lane; q < 225; q += 64) M_l[q] = p.sqrt_info[q];
    __syncthreads();
    const int li = lane & 15, lk = lane >> 4;
    v4f64 a00 = {0, 0, 0, 0}, a10 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
    imu_block_mfma(raw_l, M_l, li, lk, a00, a10, a11);
    for (int r = 0; r < 4; r++) {
        const int row = lk + 4 * r, col = li;
        G961[row * 31 + col] = a00[r];
        if (16 + row < 31) {
            G961[(16 + row) * 31 + col] = a10[r];
            G961[col * 31 + 16 + row] = a10[r];
            if (16 + col < 31) G961[(16 + row) * 31 + 16 + col] = a11[r];
        }
    }
}

// IntegrationBase::evaluate and the raw (un-whitened) Jacobian of IMUFactor::Evaluate on a caller-supplied pre-integration (P: delta state,
// jacobian, linearisation biases).  Lane 0: imu_raw_residual and imu_raw_jacobian (r15, J450 = 15 x 30 row-major, columns pose_i(6)
// speedbias_i(9) pose_j(6) speedbias_j(9)); lanes 1-4: the four imu_raw_jacobian_part calls into a 15 x 31 buffer as be_stage_imu_block_kernel
// and the solver lay it out (Jp465: column 30, which the parts do not own, keeps the value it came in with).
__global__ __launch_bounds__(64) void be_stage_imu_raw_kernel(const PreInt *P, const double *par /*pi7 sbi9 pj7 sbj9*/, double g_norm, double *r15,
                                                               double *J450, double *Jp465) {
    __shared__ double raw_l[472];
    const int lane = threadIdx.x;
    const PreInt &p = *P;
    v3 G = mk(0, 0, g_norm);
    for (int q = lane; q < 465; q += 64) raw_l[q] = Jp465[q];
    __syncthreads();
    if (lane == 0) {
        bf::imu_raw_residual(p, G, par, par + 7, par + 16, par + 23, r15);
        bf::imu_raw_jacobian(p, G, par, par + 7, par + 16, par + 23, J450);
    } else if (lane <= 4)
        bf::imu_raw_jacobian_part(p, G, par, par + 7, par + 16, par + 23, lane - 1, raw_l, 31);
    __syncthreads();
    for (int q = lane; q < 465; q += 64) Jp465[q] = raw_l[q];
}
// eval_projection_pair as the solver calls it, with the caller's cauchy / rs / ext: J is written in place over whatever the caller put there
// (2 rows of stride rs from J[0]), wgt likewise (only a cauchy call stores it).
__global__ void be_stage_projection_pair_kernel(vio_config cfg, const double *in /*pi7 pj7 ex7 inv_dep td oi9 oj9*/, int use_td, int cauchy, int rs,
                                                int ext, double *r2, double *wgt, double *J) {
    if (threadIdx.x != 0) return;
    bf::PairGeo g;
    bf::pair_geo(in, in + 7, in + 14, g);
    double ricm[9];
    stm(ricm, q2R(mkq(in[14 + 6], in[14 + 3], in[14 + 4], in[14 + 5])));
    bf::eval_projection_pair(cfg, g, ricm, in + 14, in[21], in[22], cfg.tr, in + 23, in + 32, use_td != 0, r2, J, cauchy != 0, wgt, rs, ext != 0);
}
// PoseLocalParameterization::Plus and the prior's pose delta, one thread per input: plus7[i] = pose_plus(x7[i], d6[i]), dx6[i] = pose_dx(x7[i], x07[i])
__global__ void be_stage_pose_ops_kernel(int n, const double *x7, const double *d6, const double *x07, double *plus7, double *dx6) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x[7];
    for (int k = 0; k < 7; k++) x[k] = x7[7 * i + k];
    bf::pose_plus(x, d6 + 6 * i);
    for (int k = 0; k < 7; k++) plus7[7 * i + k] = x[k];
    bf::pose_dx(x7 + 7 * i, x07 + 7 * i, dx6 + 6 * i);
}
