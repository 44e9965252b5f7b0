// What every back-end unit (be_kernels.hip, be_ingest.hip) starts from: the per-sequence context (Ctx), the phase-timer macros, namespace dm.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "be_factors.h"

using namespace dm;

// phase timers (debug): thread 0 of sequence 0 accumulates 100 MHz wall-clock ticks into B.timings[k]
#if VIO_TIMERS
#define PH_INIT long long ph_t0 = (s == 0 && threadIdx.x == 0) ? VIO_CLOCK() : 0
#define PH(k) do { if (s == 0 && threadIdx.x == 0) { long long n_ = VIO_CLOCK(); B.timings[k] += (float)(n_ - ph_t0); ph_t0 = n_; } } while (0)
#else
#define PH_INIT long long ph_t0 = 0   // (never read: the functions that tick take it as a parameter in both builds)
#define PH(k) do {} while (0)
#endif

namespace {

struct Ctx {
    float *timings;
    const DevCfg *C;
    int s, W, P, LW, NL, NLs, NPR;
    BeSeq *be;
    FeSeq *fe;
    const vio_calibration *K;   // the sequence's calibration (Batch::cal)
    PreInt *pre;
    int *lm_id, *lm_start, *lm_nobs, *lm_est, *lm_solve, *lm_dyn, *lm_order, *lm_free, *lm_tmp, *lm_pidx, *lm_aidx, *lm_relo;
    double *lm_depth, *lm_obs, *feat, *cfeat, *relo_xy, *relo_mp;
    double *H, *Sc, *Hpl, *vec, *Hll, *gl, *lvec, *res;
    int *res_lm, *res_k, *pair_start, *pair_list;
    double *pairblk, *imu_raw;
    double *prior_J, *prior_r, *prior_x0, *prior_H, *prior_rf;
    double *margA, *margB, *margV, *margW, *margE;
    int nres_cap;
};

__device__ Ctx make_ctx(const Batch &B, int s) {
    Ctx c;
    // (round 6: the dimensions come from the kernel arguments -- as fields of *B.cfg they were one dependent global round trip at the top of every
    // workgroup of every kernel before the first useful address could be formed)
    struct { int W, P, LW, NL, NP, NRES, NPRIOR, MX; } C = {B.gW, B.gP, B.gLW, B.gNL, B.gNP, B.gNRES, B.gNPRIOR, B.gMX};
    c.timings = B.timings;
    c.C = B.cfg; c.s = s; c.W = C.W; c.P = C.P; c.LW = C.LW; c.NL = C.NL; c.NLs = C.NL + 8; c.NPR = C.NPRIOR;
    c.be = B.be + s; c.fe = B.fe + s; c.K = B.cal + s;
    c.pre = B.pre + (size_t)s * (C.W + 2);
    size_t o = (size_t)s * C.NL;
    c.lm_id = B.lm_id + o; c.lm_start = B.lm_start + o; c.lm_nobs = B.lm_nobs + o; c.lm_est = B.lm_est_flag + o;
    c.lm_solve = B.lm_solve_flag + o; c.lm_dyn = B.lm_dyn + o; c.lm_order = B.lm_order + o; c.lm_free = B.lm_free + o;
    c.lm_tmp = B.lm_tmp + o; c.lm_pidx = B.lm_pidx + o; c.lm_aidx = B.lm_aidx + o; c.lm_relo = B.lm_relo + o;
    c.relo_xy = B.relo_xy + o * 2; c.relo_mp = B.relo_mp + (size_t)s * C.NP * 3;
    c.lm_depth = B.lm_depth + o; c.feat = B.para_feat + o; c.cfeat = B.cand_feat + o;
    c.lm_obs = B.lm_obs + o * (C.W + 1) * VIO_OBS_D;
    c.H = B.H + (size_t)s * C.LW * C.LW; c.Sc = B.Sc + (size_t)s * C.LW * C.LW; c.Hpl = B.Hpl + (size_t)s * (C.NL + 8) * C.LW;
    c.vec = B.vec + (size_t)s * VEC_SLOTS * C.LW;
    c.Hll = B.Hll + (size_t)s * (C.NL + 8); c.gl = B.gl + (size_t)s * (C.NL + 8); c.lvec = B.lvec + (size_t)s * (C.NL + 8) * 8;
    c.nres_cap = C.NRES;
    c.res = B.res + (size_t)s * c.nres_cap * 42;
    c.res_lm = B.res_lm + (size_t)s * c.nres_cap; c.res_k = B.res_k + (size_t)s * c.nres_cap;
    int np = (C.W + 1) * (C.W + 1);
    c.pair_start = B.pair_start + (size_t)s * (np + 1); c.pair_list = B.pair_list + (size_t)s * c.nres_cap;
    c.pairblk = B.pairblk + (size_t)s * np * 210;
    c.imu_raw = B.imu_raw + (size_t)s * C.W * 15 * 31;
    int n = C.NPRIOR;
    c.prior_J = B.prior_J + (size_t)s * n * n; c.prior_r = B.prior_r + (size_t)s * n;
    c.prior_x0 = B.prior_x0 + (size_t)s * (C.W * 7 + 17); c.prior_H = B.prior_H + (size_t)s * n * n;
    c.prior_rf = B.prior_rf + (size_t)s * n;
    int mq = 15 + n;
    c.margA = B.margA + (size_t)s * mq * mq; c.margB = B.margB + (size_t)s * mq;
    c.margV = B.margV + (size_t)s * n * n; c.margW = B.margW + (size_t)s * (n + 16) * (n + 16);
    c.margE = C.MX > 0 ? B.margE + (size_t)s * ((size_t)3 * C.MX * C.MX + (size_t)n * C.MX) : nullptr;
    return c;
}

__device__ __forceinline__ double *obs_ptr(const Ctx &c, int slot, int frame) {
    int W1 = c.W + 1;
    int ph = (frame + c.be->ring_base) % W1;
    return c.lm_obs + ((size_t)slot * W1 + ph) * VIO_OBS_D;
}
__device__ __forceinline__ bool in_problem(const Ctx &c, int slot) {
    return !c.lm_dyn[slot] && c.lm_nobs[slot] >= 2 && c.lm_start[slot] < c.W - 2;
}

}  // namespace
