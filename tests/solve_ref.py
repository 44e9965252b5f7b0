"""The solver's linearisation and trust-region step (be_phased.h: ps_setup, ps_eval / ps_evalf, ps_asm_a, ps_asm_b_schur, ps_serial, ps_ls; the
persistent be_solve kernel as a whole) by their definition, on generated window states, with the bounds of tests/test_gpu_solve_stage.py.
tests/test_solve_ref_cpu.py checks this module against itself without a GPU.  Built from factor_ref (the factors, 40-digit mpmath) and the generator
and bound helpers of marg_default_ref (make_case, prior_dx, imu_gram, proj_rows), not from the oracle and not from the kernels' order of summation.

The algorithm is Ceres' trust-region minimiser with the dogleg strategy, as optimization() configures it (DENSE_SCHUR, DOGLEG, CauchyLoss(1) on
the projection factors), written from Ceres' documentation and sources:
  cost          f = 1/2 sum rho(|r|^2): rho = identity for the prior and the IMU factors, rho(s) = log(1 + s) for the projection pairs, whose
                residual and Jacobian are scaled by sqrt(rho') = 1 / sqrt(1 + |r|^2) (Corrector: rho'' < 0 for Cauchy, so alpha = 0 and nothing
                but that scaling is applied).  An IMU factor is left out where sum_dt > 10 (estimator.cpp:1231).  The prior is the quadratic form
                1/2 c0 + dx^T r + 1/2 dx^T H dx of the marginalisation factor (c0 = 0 as staged), dx = x (-) x0.
  parameters    P = 15 (W + 1) + 7: pose k at 6 k, speed-bias k at 6 (W + 1) + 9 k, extrinsic at 15 (W + 1), td behind it; then one inverse depth per
                variable landmark.  Constant (no column): the extrinsic unless estimate_extrinsic and |Vs[0]| > 0.2; td unless estimate_td and
                !(|Vs[0]| < 0.2); without an IMU pose 0 and every speed-bias; a landmark with lm_est_flag = 1 under fix_depth.
  Jacobi        column scaling s = 1 / (1 + sqrt(diag J^T J)) of the FIRST linearisation (Solver::Options::jacobi_scaling), kept for the solve
  diagonal      D^2 = diag of the scaled J^T J, clamped to [min_lm_diagonal, max_lm_diagonal] = [1e-6, 1e32]
  Gauss-Newton  (Hs + mu D^2) y = gs with mu from min_mu = 1e-8 (DoglegStrategy; raised tenfold up to max_mu = 1 when the factorisation fails);
                in the D-scaled variables z = D y of the dogleg: gn = - D y
  dogleg        TRADITIONAL_DOGLEG in z: gradient gz = gs / D, alpha = |gz|^2 / |J D^-1 gz|^2; |gn| <= radius: gn; alpha |gz| >= radius:
                - radius gz / |gz|; otherwise the point of the segment from the Cauchy point - alpha gz to gn at distance radius.  Initial radius 1e4
                (initial_trust_region_radius).  model_cost_change = - (y^T gs + 1/2 y^T Hs y) of the step y = z / D
  step control  rho = (f - f_candidate) / model_cost_change; accepted where rho > min_relative_decrease = 1e-3; accepted: rho < 0.25 halves the
                radius, rho > 0.75 makes it max(radius, 3 |step_z|), mu = max(1e-8, 2 mu / 10); rejected: the radius is halved.  In front of
                it the parameter tolerance |dx| <= 1e-8 (|x| + 1e-8) and the function tolerance |df| <= 1e-6 f end the solve.
  candidate     Plus(x, s .* y): PoseLocalParameterization::Plus for poses and the extrinsic (factor_ref.pose_plus), addition elsewhere; an inverse
                depth of a landmark with lm_est_flag = 2 is cut at 2 / depth_max (ParameterBlock::Plus projects onto the box)
  constrained   a variable landmark with lm_est_flag = 2 makes the problem bounds-constrained: x0 goes through Plus(x0, 0) first (projected onto the
                box, quaternions re-normalised) and every step through the projected Armijo line search, f(Plus(x, a d)) <= f(x) + 1e-4 a g^T d

Precision.  Factors from factor_ref rounded to float64 (their rounding is part of the factor-level term); every sum, the scaling, the solve of the
full (unreduced) system by Gaussian elimination with partial pivoting and the dogleg in np.longdouble (64-bit mantissa); `route="mp"` forms the
sums and the solve in 40-digit mpmath instead (the CPU test finds the two equal on a W = 4 and a W = 10 case far below every bound).

Bounds (eps = 2^-52, gamma_k = k eps / (1 - k eps), C = 8, KF = 64 as in marg_default_ref).
  (a) linearisation, entrywise, as marg_default_ref bounds its reduced system: gamma_k (sum of absolute terms) + the first-order factor-level term
      (|dJ|^T |J| + |J|^T |dJ|, the IMU Gram bound, |H_prior| ddx), k = 2 nres + 15 W + n + 32 (no entry sums more products).
      cost: sum over pairs of |r| . dr / (1 + |r|^2) + 4 eps (1/2 log(1 + s)) + 2 eps (the rounding of 1 + s) + 1/2 EG[30][30] per IMU factor +
      the prior's (|r| + |H| |dx|) . ddx + gamma_(n+2) (|dx| . |r| + 1/2 |dx|^T |H| |dx|) + gamma_(nres + W + 8) (sum of absolute terms).
  (b) Gauss-Newton step.  The device solves ITS system (Mh, bh) by eliminating the landmark block (diagonal, positive) and a Cholesky
      factorisation of the Schur complement -- block elimination of a positive definite matrix and Cholesky are backward stable: the returned y
      satisfies (Mh + dM) y = bh with |dM| <= C N eps d d^T, d = sqrt(diag M), N the order (Higham, Accuracy and Stability, 10.1 with
      |L| |L^T| <= d d^T; the convention of marg_ref).  Against the reference's (M, b): r = M y - b = (M - Mh - dM) y + (bh - b), so entrywise
          |r| <= (EM + C N eps d d^T) |y| + Eb,
      EM_ab = s_a s_b EH_ab + |Hs_ab| (q_a + q_b + 3 eps) + [a = b] mu (EM_aa + 3 eps D_a^2), q_a = EH_aa / (2 H_aa) + 3 eps the relative error of
      s_a (d s / s <= 1/2 dh / h), Eb_a = s_a Eg_a + |gs_a| (q_a + eps): the linearisation bounds of (a) carried through the scaling.
      Forward: y - y_ref = M^-1 r exactly, so |y - y_ref| <= |M^-1| rbound(|y_ref|) / (1 - C N eps kappa), kappa = cond_2 of M scaled to unit
      diagonal, asserted only where C N eps kappa <= 1e-3 (the other cases by name in the CPU test).
      U, the landmark part of the Schur complement the first slot leaves in Sc: U_ab = sum_k w_k h_ka h_kb, w_k = s_k^2 / (s_k^2 Hll_k + mu D_k^2):
      sum_k w_k (|dh_ka| |h_kb| + |h_ka| |dh_kb|) + |w_k h_ka h_kb| (3 EHll_k / Hll_k + 20 eps) + gamma_(Fa + 8) sum_k |w_k h_ka h_kb|.
  (c) dogleg step, dogleg_norm, model_change, alpha.  The propagation of (a), (b) through alpha, the branch and the interpolation is not derived; per
      the project's rule the bar is 16 times what float64 numpy of this definition leaves against the extended-precision one -- here the worst of
      three evaluations with the residuals summed in three different orders, numpy.linalg.solve for the step, and every factor (Jacobian and
      residual entries, IMU Gram blocks, the prior's gradient) moved by its factor-level bound with random signs: the reference's factors are exact
      to float64 rounding, a float64 evaluation of them is allowed KF eps scale (tests/test_gpu_factor_edges.py), and without that term the bar
      of a Cauchy step would be a few eps.  Per case, radius and quantity, max-norm.  Measured (CPU test): those float64 evaluations differ from the reference by
      1e-11 .. 5.7e-2 of the largest step entry, median 5e-7 (the Gauss-Newton branch has the derived bound of (b) instead; dogleg_norm on the
      interpolated branch the one derived in dogleg()).
      Xc: factor_ref.pose_plus at x0 and the step the device returned (fl(s stp)): KF eps scale, entrywise; exact for the additive blocks
      up to one rounding.
  (d) ccost: the definition's cost at the candidate the device returned, within the cost bound of (a) there.  Decision and radius: exact."""

import mpmath
import numpy as np

import factor_ref as fr
import marg_default_ref as D
import marg_ref as mr

L = np.longdouble
EPS, C, KF, gamma = D.EPS, D.C, D.KF, D.gamma
MIN_DIAG, MAX_DIAG, MU0, RADIUS0, MIN_REL_DECREASE = 1e-6, 1e32, 1e-8, 1e4, 1e-3
PS_FUSE_CAP = 256


# ------------------------------------------------------------------------------------------------------------ cached factors
def _key(*a):
    return tuple(np.ascontiguousarray(x, np.float64).tobytes() if not isinstance(x, (bool, tuple)) else x for x in a)


_proj_cache, _res_cache, _gram_cache, _cinv_cache = {}, {}, {}, {}


def proj_rows(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    k = _key(K, pi, pj, ex, inv_dep, td, oi, oj, bool(use_td))
    if k not in _proj_cache:
        _proj_cache[k] = D.proj_rows(K, pi, pj, ex, inv_dep, td, oi, oj, use_td)
    return _proj_cache[k]


def proj_res(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    k = _key(K, pi, pj, ex, inv_dep, td, oi, oj, bool(use_td))
    if k in _proj_cache:
        return _proj_cache[k][5], _proj_cache[k][6]
    if k not in _res_cache:
        _res_cache[k] = fr.proj_residual(K, pi, pj, ex, inv_dep, td, oi, oj, use_td)
    return _res_cache[k]


def imu_gram(cfg, pre, ns, pi, sbi, pj, sbj):
    k = (id(pre),) + _key(pi, sbi, pj, sbj)
    if k not in _gram_cache:
        _gram_cache[k] = D.imu_gram(cfg, pre, ns, pi, sbi, pj, sbj)
    return _gram_cache[k]


def imu_cost(cfg, pre, ns, pi, sbi, pj, sbj):
    """1/2 r^T C^-1 r of an IMU factor and its bound (the [30][30] entry of marg_default_ref.imu_gram's), without the Jacobian"""
    k = (id(pre),) + _key(pi, sbi, pj, sbj)
    if k in _gram_cache:
        G, EG, _ = _gram_cache[k]
        return L(0.5) * L(G[30, 30]), 0.5 * EG[30, 30]
    rr, rs = fr.imu_residual(pre, float(cfg.g_norm), pi, sbi, pj, sbj)
    rs = np.maximum(rs, np.r_[np.full(3, pre["scale_p"]), np.ones(3), np.full(3, pre["scale_v"]), np.zeros(6)])
    if id(pre) not in _cinv_cache:
        with mpmath.workdps(fr.DPS):
            Cm = fr._mpm(pre["cov"])
            Cm = (Cm + Cm.T) / 2
            cov = 0.5 * (pre["cov"] + pre["cov"].T)
            dc = 1.0 / np.sqrt(np.diag(cov))
            ev = np.linalg.eigvalsh(cov * np.outer(dc, dc))
            _cinv_cache[id(pre)] = (Cm ** -1, dc, float(ev[0]), float(ev[-1] / ev[0]), pre)
    Ci, dc, lmin, kappa, _ = _cinv_cache[id(pre)]
    with mpmath.workdps(fr.DPS):
        v = mpmath.matrix([mpmath.mpf(float(x)) for x in rr])
        c2 = (v.T * Ci * v)[0, 0]
        hi = float(c2)
        cost = L(0.5) * (L(hi) + L(float(c2 - mpmath.mpf(hi))))
    e_col = C * (ns + 1) * KF * EPS * float(np.linalg.norm(rs * dc)) / np.sqrt(lmin)
    sg = float(np.sqrt(2.0 * float(cost)))
    return cost, 0.5 * (2 * e_col * sg + C * (ns + 31) * EPS * kappa * sg * sg)


# ------------------------------------------------------------------------------------------------------------ the problem
class Problem:
    """What of a staged state the solver sees: the landmarks in the problem, the variable ones, the residual list, the active parameters"""

    def __init__(self, case, cfg):
        st, W = case["st"], case["W"]
        self.case, self.cfg, self.st, self.W, self.W1 = case, cfg, st, W, W + 1
        self.P = 15 * (W + 1) + 7
        self.oS, self.oE, self.oT = 6 * (W + 1), 15 * (W + 1), 15 * (W + 1) + 6
        order = [int(s) for s in st["lm_order"][:int(st.get("n_lm", len(st["lm_order"])))]]
        self.plist = [s for s in order if D._in_problem(st, s, W)]
        self.var = [k for k, s in enumerate(self.plist) if not (st["lm_est_flag"][s] == 1 and cfg.fix_depth)]
        self.alist = [self.plist[k] for k in self.var]
        self.F, self.Fa = len(self.plist), len(self.var)
        self.aidx = {k: a for a, k in enumerate(self.var)}
        self.res = [(k, int(st["lm_start"][s]), int(st["lm_start"][s]) + q) for k, s in enumerate(self.plist) for q in range(1, int(st["lm_nobs"][s]))]
        self.nres = len(self.res)
        v0 = float(np.linalg.norm(np.asarray(st["Vs"][0], L)))
        self.use_imu = bool(cfg.use_imu)
        self.ex_active = bool(cfg.estimate_extrinsic) and v0 > 0.2
        self.td_active = self.use_imu and bool(cfg.estimate_td) and not (v0 < 0.2)
        self.vext = self.ex_active or self.td_active
        act = np.ones(self.P, bool)
        act[self.oE:self.oE + 6], act[self.oT] = self.ex_active, self.td_active
        if not self.use_imu:
            act[:6], act[self.oS:self.oE] = False, False
        self.act = np.flatnonzero(act)
        self.ub = 2.0 / float(cfg.depth_max)
        self.bounded = [a for a, s in enumerate(self.alist) if st["lm_est_flag"][s] == 2]
        self.constrained = len(self.bounded) > 0
        self.pair_counts = {}
        for _, i, j in self.res:
            self.pair_counts[(i, j)] = self.pair_counts.get((i, j), 0) + 1

    def x0(self):
        """the staged point: (X, feat); a constrained problem's is projected onto the box (Plus(x0, 0): quaternion renormalisation is below 1 eps here)"""
        feat = np.array([1.0 / float(self.st["lm_depth"][s]) for s in self.plist])
        if self.constrained:
            for a in self.bounded:
                feat[self.var[a]] = min(feat[self.var[a]], self.ub)
        return self.case["X"], feat

    def obs(self, slot, f):
        return self.st["lm_obs"][slot, (f + int(self.st["ring_base"])) % self.W1]

    def prior_map(self, a):
        W = self.W
        if a < 6 * W:
            return a
        if a < 6 * W + 9:
            return self.oS + (a - 6 * W)
        if a < 6 * W + 15:
            return self.oE + (a - 6 * W - 9)
        return self.oT


class Lin:
    pass


def cost(pb, X, feat):
    """(f, bound): the cost at (X, feat) by the definition"""
    return linearise(pb, X, feat, jac=False)


def linearise(pb, X, feat, jac=True, route="ld", order=None, f64=False, rng=None):
    """The definition's linearisation at (X, feat): Lin with cost, H [P, P], g [P], Hpl [Fa, P], Hll, gl [Fa] (np.longdouble, or mpmath objects for
    route = "mp") and the entrywise bounds E* (float64).  jac = False: (cost, bound) only.  f64 = True: every sum in float64 numpy, residuals in the
    given order and, with rng, every factor moved by its factor-level bound with random signs (the measurement of (c)): plain arrays."""
    cfg, st, W, W1, P, Fa = pb.cfg, pb.st, pb.W, pb.W1, pb.P, pb.Fa
    K, use_td = fr.proj_consts(cfg), bool(cfg.estimate_td)
    n = 6 * W + 16
    cv = (lambda a: np.asarray(a, np.float64)) if f64 else mr.to_mp if route == "mp" else (lambda a: np.asarray(a, np.float64).astype(L))
    like = cv(np.zeros(1))
    f, Ef, absf = like[0] * 0, 0.0, 0.0
    if jac:
        H, g = mr._zeros((P, P), like), mr._zeros(P, like)
        Hpl, Hll, gl = mr._zeros((Fa, P), like), mr._zeros(Fa, like), mr._zeros(Fa, like)
        aH, ag, aHpl, aHll, agl = np.zeros((P, P)), np.zeros(P), np.zeros((Fa, P)), np.zeros(Fa), np.zeros(Fa)
        EH, Eg, EHpl, EHll, Egl = np.zeros((P, P)), np.zeros(P), np.zeros((Fa, P)), np.zeros(Fa), np.zeros(Fa)
    weights = []
    # ---- prior
    prior = st["prior"]
    if prior is not None:
        Hp, rp, x0 = np.asarray(prior["H"], np.float64), np.asarray(prior["r"], np.float64), np.asarray(prior["x0"], np.float64)
        dx, sdx, _ = D.prior_dx(X, x0, prior["present"], W, cv)
        idx = np.array([pb.prior_map(a) for a in range(n)])
        Hc, dxc, rc = cv(Hp), cv(dx), cv(rp)
        grad = rc + Hc @ dxc
        f = f + dxc @ rc + (dxc @ (Hc @ dxc)) / 2
        ddx = KF * EPS * sdx
        agrad = np.abs(rp) + np.abs(Hp) @ np.abs(dx)
        if rng is not None:
            grad = grad + rng.choice([-1.0, 1.0], n) * (np.abs(Hp) @ ddx)
        Ef += float(agrad @ ddx) + gamma(n + 2) * float(np.abs(dx) @ np.abs(rp) + 0.5 * np.abs(dx) @ np.abs(Hp) @ np.abs(dx))
        absf += abs(float(dx @ rp)) + 0.5 * abs(float(dx @ Hp @ dx))
        if jac:
            H[np.ix_(idx, idx)] = H[np.ix_(idx, idx)] + Hc
            g[idx] = g[idx] + grad
            aH[np.ix_(idx, idx)] += np.abs(Hp)
            ag[idx] += agrad
            Eg[idx] += gamma(n + 1) * agrad + np.abs(Hp) @ ddx
    # ---- IMU factors
    sum_dt = []
    if pb.use_imu:
        for i in range(W):
            pre, ns = D.imu_pre(cfg, st, i + 1)
            sum_dt.append(pre["sum_dt"])
            if pre["sum_dt"] > 10.0:
                continue
            a4 = (cfg, pre, ns, X["pose"][i], X["sb"][i], X["pose"][i + 1], X["sb"][i + 1])
            if not jac:
                c1, e1 = imu_cost(*a4)
                f, Ef, absf = f + c1, Ef + e1, absf + float(c1)      # (cost-only evaluations run in np.longdouble)
                continue
            G, EG, _ = imu_gram(*a4)
            ii = np.r_[6 * i + np.arange(6), pb.oS + 9 * i + np.arange(9), 6 * (i + 1) + np.arange(6), pb.oS + 9 * (i + 1) + np.arange(9)]
            if rng is not None:
                sg_ = np.triu(rng.choice([-1.0, 1.0], (31, 31)))
                G = G + (sg_ + np.triu(sg_, 1).T) * EG
            Gc = cv(G)
            H[np.ix_(ii, ii)] = H[np.ix_(ii, ii)] + Gc[:30, :30]
            g[ii] = g[ii] + Gc[:30, 30]
            f = f + Gc[30, 30] / 2
            aH[np.ix_(ii, ii)] += np.abs(G[:30, :30])
            ag[ii] += np.abs(G[:30, 30])
            EH[np.ix_(ii, ii)] += EG[:30, :30]
            Eg[ii] += EG[:30, 30]
            Ef += 0.5 * EG[30, 30]
            absf += 0.5 * G[30, 30]
    # ---- projection pairs
    for q in (range(pb.nres) if order is None else order):
        k, i, j = pb.res[q]
        slot = pb.plist[k]
        a9 = (K, X["pose"][i], X["pose"][j], X["ex"], float(feat[k]), X["td"], pb.obs(slot, i), pb.obs(slot, j), use_td)
        if jac:
            wJ, dJ, wr, dr, w, r2, r2s = proj_rows(*a9)
            weights.append(w)
            if rng is not None:
                wJ, wr = wJ + rng.choice([-1.0, 1.0], wJ.shape) * dJ, wr + rng.choice([-1.0, 1.0], 2) * dr
        else:
            r2, r2s = proj_res(*a9)
        s2 = float(r2 @ r2)
        if f64:
            f = f + 0.5 * np.log1p(s2)
        elif route == "mp":
            with mpmath.workdps(fr.DPS):
                f = f + mpmath.log(1 + mpmath.mpf(float(r2[0])) ** 2 + mpmath.mpf(float(r2[1])) ** 2) / 2
        else:
            f = f + np.log1p(L(r2[0]) * L(r2[0]) + L(r2[1]) * L(r2[1])) / 2
        half = 0.5 * float(np.log1p(s2))
        Ef += float(np.abs(r2) @ (KF * EPS * r2s)) / (1.0 + s2) + 4 * EPS * half + 2 * EPS
        absf += half
        if not jac:
            continue
        pc = np.r_[6 * i + np.arange(6), 6 * j + np.arange(6), pb.oE + np.arange(6), pb.oT]
        Jp, Jc, rc = wJ[:, :19], cv(wJ[:, :19]), cv(wr)
        H[np.ix_(pc, pc)] = H[np.ix_(pc, pc)] + Jc.T @ Jc
        g[pc] = g[pc] + Jc.T @ rc
        aJ, adJ = np.abs(Jp), dJ[:, :19]
        aH[np.ix_(pc, pc)] += aJ.T @ aJ
        ag[pc] += aJ.T @ np.abs(wr)
        EH[np.ix_(pc, pc)] += adJ.T @ aJ + aJ.T @ adJ
        Eg[pc] += adJ.T @ np.abs(wr) + aJ.T @ dr
        if k in pb.aidx:
            a = pb.aidx[k]
            Jl, al, dl = cv(wJ[:, 19]), np.abs(wJ[:, 19]), dJ[:, 19]
            Hpl[a, pc] = Hpl[a, pc] + Jl @ Jc
            Hll[a] = Hll[a] + Jl @ Jl
            gl[a] = gl[a] + Jl @ rc
            aHpl[a, pc] += al @ aJ
            aHll[a] += al @ al
            agl[a] += al @ np.abs(wr)
            EHpl[a, pc] += dl @ aJ + al @ adJ
            EHll[a] += 2 * (al @ dl)
            Egl[a] += dl @ np.abs(wr) + al @ dr
    Ef += gamma(pb.nres + W + 8) * absf
    if not jac:
        return f, Ef
    r = Lin()
    r.cost, r.cost_bound = f, Ef
    r.H, r.g, r.Hpl, r.Hll, r.gl = H, g, Hpl, Hll, gl
    terms = 2 * pb.nres + 15 * W + n + 32
    gt = gamma(terms)
    r.EH, r.Eg, r.EHpl, r.EHll, r.Egl = EH + gt * aH, Eg + gt * ag, EHpl + gt * aHpl, EHll + gt * aHll, Egl + gt * agl
    r.weights, r.sum_dt, r.terms = weights, sum_dt, terms
    return r


# ------------------------------------------------------------------------------------------------------------ the step
def ld_inverse(M):
    """inverse by Gauss-Jordan elimination with partial pivoting in np.longdouble, one rank-one update per pivot"""
    k = M.shape[0]
    A = np.zeros((k, 2 * k), L)
    A[:, :k] = M
    A[np.arange(k), k + np.arange(k)] = 1
    for c in range(k):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        col = A[:, c].copy()
        col[c] = 0
        A -= np.outer(col, A[c])
    return A[:, k:].copy()


class Step:
    pass


def _full(pb, lin, xp=np):
    """the unreduced system over [active parameters | variable landmarks] from a linearisation"""
    act, na, Fa = pb.act, len(pb.act), pb.Fa
    N = na + Fa
    Hf = mr._zeros((N, N), np.asarray(lin.H))
    Hf[:na, :na] = lin.H[np.ix_(act, act)]
    Hf[na:, :na] = lin.Hpl[:, act]
    Hf[:na, na:] = lin.Hpl[:, act].T
    for a in range(Fa):
        Hf[na + a, na + a] = lin.Hll[a]
    gf = np.concatenate([lin.g[act], lin.gl])
    return Hf, gf


def scaling(pb, lin):
    """Jacobi column scaling of a (first) linearisation over the full variable vector, np.longdouble"""
    Hf, _ = _full(pb, lin)
    return 1 / (1 + np.sqrt(np.diag(Hf).astype(L)))


def gn_system(pb, lin, s, mu=MU0, q=None):
    """Step with the scaled, regularised system M y = b, its exact solution y, M^-1, the trust-region diagonal D and the bounds of (b).
    q: the relative error bound of s where s is kept from an EARLIER linearisation (a later iteration of a solve); None: s is this one's"""
    Hf, gf = _full(pb, lin)
    Hf, gf = D._as_ld(Hf), D._as_ld(gf)
    na, N = len(pb.act), len(gf)
    r = Step()
    r.s, r.N, r.na, r.mu = s, N, na, mu
    r.Hs = Hf * np.outer(s, s)
    r.gs = gf * s
    d2 = np.minimum(np.maximum(np.diag(r.Hs), L(MIN_DIAG)), L(MAX_DIAG))
    r.Dg = np.sqrt(d2)
    r.M = r.Hs + np.diag(L(mu) * d2)
    r.Mi = ld_inverse(r.M)
    r.y = r.Mi @ r.gs
    r.gn = -r.Dg * r.y
    # ---- bounds
    EHf = np.zeros((N, N))
    EHf[:na, :na] = lin.EH[np.ix_(pb.act, pb.act)]
    EHf[na:, :na] = lin.EHpl[:, pb.act]
    EHf[:na, na:] = lin.EHpl[:, pb.act].T
    EHf[na + np.arange(N - na), na + np.arange(N - na)] = lin.EHll
    Egf = np.concatenate([lin.Eg[pb.act], lin.Egl])
    sf, Hsf, hd = D._f64(s), np.abs(D._f64(r.Hs)), np.abs(D._f64(np.diag(Hf)))
    if q is None:
        q = np.where(hd > 0, np.diag(EHf) / (2 * np.where(hd > 0, hd, 1.0)), 0.0) + 3 * EPS
    EM = np.outer(sf, sf) * EHf + Hsf * (q[:, None] + q[None, :] + 3 * EPS)
    di = np.arange(N)
    EM[di, di] += mu * (EM[di, di] + 3 * EPS * D._f64(d2))
    r.q = q                                    # relative error bound of the column scaling
    r.EM, r.Eb = EM, sf * Egf + np.abs(D._f64(r.gs)) * (q + EPS)
    r.dd = np.sqrt(np.abs(D._f64(np.diag(r.M))))
    Msc = D._f64(r.M) / np.outer(r.dd, r.dd)
    ev = np.linalg.eigvalsh(0.5 * (Msc + Msc.T))
    r.kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    r.rho_fwd = C * N * EPS * r.kappa
    r.fwd_bounded = bool(r.rho_fwd <= 1e-3)
    r.y_bound = (np.abs(D._f64(r.Mi)) @ r.res_bound_of(np.abs(D._f64(r.y)))) / (1 - r.rho_fwd) if r.fwd_bounded else None
    return r


def _res_bound_of(self, ay):
    return (self.EM + C * self.N * EPS * np.outer(self.dd, self.dd)) @ ay + self.Eb


Step.res_bound_of = _res_bound_of


def schur_u(pb, lin, s, mu=MU0):
    """U = sum_k w_k h_k h_k^T over the parameter columns (unscaled), w_k = s_k^2 / (s_k^2 Hll_k + mu D_k^2), and its entrywise bound"""
    na, Fa, P = len(pb.act), pb.Fa, pb.P
    sl = s[na:]
    Hll, Hpl = D._as_ld(lin.Hll), D._as_ld(lin.Hpl)
    hl = sl * sl * Hll
    d2 = np.minimum(np.maximum(hl, L(MIN_DIAG)), L(MAX_DIAG))
    w = sl * sl / (hl + L(mu) * d2)
    U = (Hpl * w[:, None]).T @ Hpl
    wf, h, dh = D._f64(w), np.abs(D._f64(Hpl)), lin.EHpl
    hll = np.abs(D._f64(Hll))
    rel = 3 * np.where(hll > 0, lin.EHll / np.where(hll > 0, hll, 1.0), 0.0) + 20 * EPS
    aU = (h * wf[:, None]).T @ h
    EU = (dh * wf[:, None]).T @ h + (h * wf[:, None]).T @ dh + (h * (wf * rel)[:, None]).T @ h + gamma(Fa + 8) * aU
    return U, EU, w


def schur_s(st):
    """The reference's Schur complement of a gn_system over the active parameters, S = M_pp - M_pl M_ll^-1 M_lp (M_ll is diagonal), and its
    entrywise bound: EM_pp + sum_k (EM_ak |M_bk| + |M_ak| EM_bk) / M_kk + |M_ak M_bk| EM_kk / M_kk^2, + gamma_(Fa+8) of the absolute terms"""
    na, N = st.na, st.N
    Mpp, Mlp, dl = st.M[:na, :na], st.M[na:, :na], np.diag(st.M)[na:]
    S = Mpp - (Mlp / dl[:, None]).T @ Mlp if N > na else Mpp.copy()
    ES = st.EM[:na, :na].copy()
    aS = np.abs(D._f64(Mpp))
    if N > na:
        A, dA, d, dd_ = np.abs(D._f64(Mlp)), st.EM[na:, :na], D._f64(dl), np.diag(st.EM)[na:]
        ES += (dA / d[:, None]).T @ A + (A / d[:, None]).T @ dA + (A * (dd_ / d ** 2)[:, None]).T @ A
        aS = aS + (A / d[:, None]).T @ A
    return S, ES + gamma(N - na + 8) * aS


def gauge_fix(X0, X):
    """double2vector (estimator.cpp:985-1111) in IMU mode, in np.longdouble: the solved window turned about the vertical by the yaw that frame 0
    lost, yaw(R0 staged) - yaw(R0 solved) (Utility::R2ypr: atan2(R10, R00)), and moved so that frame 0 keeps its position.
    Returns (P [W+1, 3], R [W+1, 3, 3], V [W+1, 3])"""
    def rot(q):
        x, y, z, w = [L(float(v)) for v in q]
        n = np.sqrt(x * x + y * y + z * z + w * w)
        x, y, z, w = x / n, y / n, z / n, w / n
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], L)
    R0, R00 = rot(X0["pose"][0, 3:]), rot(X["pose"][0, 3:])
    dy = np.arctan2(R0[1, 0], R0[0, 0]) - np.arctan2(R00[1, 0], R00[0, 0])
    c, s_ = np.cos(dy), np.sin(dy)
    Rd = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]], L)
    W1 = X["pose"].shape[0]
    Pn = np.array([Rd @ (X["pose"][i, :3].astype(L) - X["pose"][0, :3].astype(L)) + X0["pose"][0, :3].astype(L) for i in range(W1)])
    Rn = np.array([Rd @ rot(X["pose"][i, 3:]) for i in range(W1)])
    Vn = np.array([Rd @ X["sb"][i, :3].astype(L) for i in range(W1)])
    return Pn, Rn, Vn


def dogleg(st, radius):
    """the traditional dogleg step of a gn_system at the given radius: dict(branch, z, y, norm, model_change, alpha, r_gn, r_cauchy)"""
    gz = st.gs / st.Dg
    sg = gz / st.Dg
    gnorm = np.sqrt(gz @ gz)
    alpha = (gz @ gz) / (sg @ (st.Hs @ sg))
    r_gn, r_c = np.sqrt(st.gn @ st.gn), alpha * gnorm
    if r_gn <= radius:
        branch, z = "gn", st.gn.copy()
    elif r_c >= radius:
        branch, z = "cauchy", -(L(radius) / gnorm) * gz
    else:
        a, b = -alpha * gz, st.gn
        d = b - a
        aa, ad, dd_ = a @ a, a @ d, d @ d
        beta = (-ad + np.sqrt(ad * ad + dd_ * (L(radius) ** 2 - aa))) / dd_
        branch, z = "interp", a + beta * d
        # |z| = radius whatever a and d are: only the rounding of beta moves it.  beta solves aa + 2 beta ad + beta^2 dd = R^2; with every
        # inner product off by gamma_N of its sum of absolute terms, (2 ad + 2 beta dd) dbeta = 2 sqrt(disc) dbeta <= gamma (aa + 2 beta
        # sqrt(aa dd) + beta^2 dd + R^2), and d|z| <= |d| dbeta + gamma |z|
        gN = gamma(len(z) + 16)
        disc = ad * ad + dd_ * (L(radius) ** 2 - aa)
        dbeta = gN * float(aa + 2 * beta * np.sqrt(aa * dd_) + beta * beta * dd_ + L(radius) ** 2) / float(2 * np.sqrt(disc))
        norm_bound = float(np.sqrt(dd_)) * dbeta + gN * radius
    y = z / st.Dg
    if branch != "interp":
        norm_bound = None
    return dict(norm_bound=norm_bound, branch=branch, z=z, y=y, norm=np.sqrt(z @ z), model_change=-(y @ st.gs + (y @ (st.Hs @ y)) / 2), alpha=alpha, r_gn=r_gn, r_cauchy=r_c)


def radii(st):
    """three radii, one per branch, each at least a factor 2 from a branch point (None where the branch points are closer than a factor 4)"""
    d = dogleg(st, RADIUS0)
    r1, r2 = float(d["r_gn"]), float(d["r_cauchy"])
    return dict(gn=RADIUS0 if RADIUS0 >= 2 * r1 else 2 * r1, cauchy=0.5 * r2, interp=float(np.sqrt(r1 * r2)) if r1 >= 4 * r2 else None), r1, r2


def candidate(pb, X, feat, s, y, a=1.0):
    """Plus(x, a s y) by the definition: (Xc, cfeat, delta over P, landmark step)"""
    na = len(pb.act)
    delta = np.zeros(pb.P)
    delta[pb.act] = D._f64(L(a) * (s[:na] * y[:na]))
    dl = D._f64(L(a) * (s[na:] * y[na:]))
    return plus(pb, X, feat, delta, dl) + (delta, dl)


def plus(pb, X, feat, delta, dl):
    """Plus(x, delta) for a float64 tangent step: poses and the extrinsic through factor_ref.pose_plus, the rest additive, the box of the bounded
    landmarks.  Returns (Xc, cfeat, scale of Xc's pose entries as a dict like Xc)"""
    W1 = pb.W1
    Xc = dict(pose=X["pose"].copy(), sb=X["sb"].copy(), ex=X["ex"].copy(), td=X["td"])
    sc = dict(pose=np.zeros((W1, 7)), ex=np.zeros(7))
    act = np.zeros(pb.P, bool)
    act[pb.act] = True
    for k in range(W1):
        if act[6 * k]:
            Xc["pose"][k], sc["pose"][k] = fr.pose_plus(X["pose"][k], delta[6 * k:6 * k + 6])
        if act[pb.oS + 9 * k]:
            Xc["sb"][k] = X["sb"][k] + delta[pb.oS + 9 * k:pb.oS + 9 * k + 9]
    if pb.ex_active:
        Xc["ex"], sc["ex"] = fr.pose_plus(X["ex"], delta[pb.oE:pb.oE + 6])
    if pb.td_active:
        Xc["td"] = X["td"] + delta[pb.oT]
    cf = np.array(feat, np.float64).copy()
    for a, k in enumerate(pb.var):
        cf[k] = feat[k] + dl[a]
        if a in pb.bounded:
            cf[k] = min(cf[k], pb.ub)
    return Xc, cf, sc


def step_control(f0, fc, model_change, radius, dogleg_norm):
    """(accepted, new radius, rho) by the rule of the docstring"""
    rho = float((f0 - fc) / model_change)
    if not rho > MIN_REL_DECREASE:
        return False, 0.5 * radius, rho
    r = radius
    if rho < 0.25:
        r = 0.5 * r
    if rho > 0.75:
        r = max(r, 3.0 * dogleg_norm)
    return True, r, rho


# ------------------------------------------------------------------------------------------------------------ float64 numpy (the measurement of (c))
def np_step(pb, X, feat, radius, seed, perturb=True):
    """the definition in float64 numpy with the residuals summed in a shuffled order and (perturb) every factor moved by its factor-level bound
    -- what the factor tests allow a float64 evaluation of the factors to differ by -- with random signs: dict(z, norm, model_change, y_gn)"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(pb.nres)
    lin = linearise(pb, X, feat, order=order, f64=True, rng=rng if perturb else None)
    Hf, gf = _full(pb, lin)
    s = 1.0 / (1.0 + np.sqrt(np.diag(Hf)))
    Hs, gs = Hf * np.outer(s, s), gf * s
    d2 = np.clip(np.diag(Hs), MIN_DIAG, MAX_DIAG)
    Dg = np.sqrt(d2)
    y = np.linalg.solve(Hs + np.diag(MU0 * d2), gs)
    st = Step()
    st.gs, st.Dg, st.Hs, st.gn = gs.astype(L), Dg.astype(L), Hs.astype(L), (-Dg * y).astype(L)
    # (the branch logic once more, in float64)
    gz = gs / Dg
    sg = gz / Dg
    gnorm = np.sqrt(gz @ gz)
    alpha = (gz @ gz) / (sg @ (Hs @ sg))
    gn = -Dg * y
    r_gn = np.sqrt(gn @ gn)
    if r_gn <= radius:
        z = gn
    elif alpha * gnorm >= radius:
        z = -(radius / gnorm) * gz
    else:
        a, d = -alpha * gz, gn + alpha * gz
        aa, ad, dd_ = a @ a, a @ d, d @ d
        z = a + (-ad + np.sqrt(ad * ad + dd_ * (radius * radius - aa))) / dd_ * d
    yy = z / Dg
    return dict(z=z, norm=float(np.sqrt(z @ z)), model_change=float(-(yy @ gs + 0.5 * yy @ Hs @ yy)), y_gn=y, lin=lin, alpha=float(alpha))


def bars(pb, X, feat, st, radius):
    """(c): 16 times the worst difference of three float64 numpy evaluations from the extended-precision step: dict(z, norm, model_change, alpha)"""
    ref = dogleg(st, radius)
    out = dict(z=0.0, norm=0.0, model_change=0.0, alpha=0.0)
    for seed in (1, 2, 3):
        e = np_step(pb, X, feat, radius, seed)
        out["z"] = max(out["z"], float(np.max(np.abs(e["z"].astype(L) - ref["z"]))))
        out["norm"] = max(out["norm"], abs(float(L(e["norm"]) - ref["norm"])))
        out["model_change"] = max(out["model_change"], abs(float(L(e["model_change"]) - ref["model_change"])))
        out["alpha"] = max(out["alpha"], abs(float(L(e["alpha"]) - ref["alpha"])))
    measured = out["z"]
    out = {k: 16.0 * v for k, v in out.items()}
    out["z_measured"] = measured                               # the float64 difference itself (max-norm), for the record of the CPU test
    if ref["branch"] == "interp":
        out["norm"] = max(out["norm"], ref["norm_bound"])       # (derived in dogleg(): the float64 evaluations land on the radius to an ulp by luck)
    if ref["branch"] == "gn" and st.fwd_bounded:
        # the Gauss-Newton branch has a derived bound: z = - D y, |dz| <= D |dy| + |y| dD with (b)'s forward bound and dD = 1/2 EM_aa / D + 3 eps D
        Dg = D._f64(st.Dg)
        out["z"] = Dg * st.y_bound + np.abs(D._f64(st.y)) * (0.5 * np.diag(st.EM) / Dg + 3 * EPS * Dg)
    return out, ref


# ------------------------------------------------------------------------------------------------------------ the cases
def _fill(W, nres, base):
    """extra landmarks (start 0) that bring the residual count from `base` to `nres`: tracks of W observations first, one shorter one at the end"""
    out, need = [], nres - base
    assert need >= 0
    while need > 0:
        m = min(W, need)                      # residuals of this landmark = nobs - 1 <= W
        out.append((0, m + 1, 0))
        need -= m
    return out


def std_nres(W, F0):
    """residuals of marg_default_ref.make_case's standard landmarks that are in the problem: F0 from frame 0 (the generator's lengths), (1, 3), (1, W)"""
    W1 = W + 1
    nobs = [W1 if li % 3 == 2 else 2 + (li + (li // 3)) % (W1 - 1) for li in range(F0)]
    if F0:
        nobs[F0 - 1] = W1
    if 1 < W - 2:
        nobs += [min(3, W1 - 1), W]
    return sum(n - 1 for n in nobs)


def _nres_case(W, nres, seed, **kw):
    return dict(kw, W=W, F0=5, seed=seed, extra_spec=tuple(_fill(W, nres, std_nres(W, 5))))


CASES = {
    # name: (kwargs of make_case, configuration beyond the window size, post-processing, handles)
    "base_W4": (dict(W=4, F0=5, seed=1, ring_base=2, rot_pre=1), {}, {}),
    "base_W10": (dict(W=10, F0=17, seed=2, ring_base=3, rot_pre=4), {}, {}),
    "big_W11": (dict(W=11, F0=9, seed=3, ring_base=5, rot_pre=2), {}, {}),
    "big_W20": (dict(W=20, F0=12, seed=4, ring_base=11, rot_pre=13), {}, {}),
    "no_prior_W4": (dict(W=4, F0=6, seed=5, prior=None, ring_base=1), {}, {}),
    "absent_W10": (dict(W=10, F0=9, seed=6, prior="absent", moved=1, ring_base=7, rot_pre=3), {}, {}),
    "moved_W4": (dict(W=4, F0=7, seed=7, moved=1, ring_base=3), {}, {}),
    "long_dt_W4": (dict(W=4, F0=6, seed=8, long_dt=1, prior=None, ring_base=1), {}, {}),
    "outlier_W4": (dict(W=4, F0=8, seed=9, outlier=1, ring_base=4), {}, {}),
    "no_imu_W4": (dict(W=4, F0=8, seed=10, use_imu=0, prior=None, ring_base=2), dict(use_imu=0), {}),
    "noshuffle_W4": (dict(W=4, F0=6, seed=11, shuffle=0), {}, {}),
    "ex_td_fast_W4": (dict(W=4, F0=8, seed=12, estimate_td=1, tr=0.02, ring_base=1), dict(estimate_extrinsic=1, estimate_td=1, tr=0.02), {}),
    "ex_td_slow_W4": (dict(W=4, F0=8, seed=12, estimate_td=1, tr=0.02, ring_base=1), dict(estimate_extrinsic=1, estimate_td=1, tr=0.02), dict(v0_scale=0.25)),
    "two_frames_W10": (dict(W=10, F0=4, seed=13, ring_base=2, extra_spec=((3, 2, 0), (5, 2, 0))), {}, {}),
    "pair64_W10": (dict(W=10, F0=3, seed=14, ring_base=6, extra_spec=tuple([(2, 2, 0)] * 64)), {}, {}),
    "pair65_W10": (dict(W=10, F0=3, seed=14, ring_base=6, extra_spec=tuple([(2, 2, 0)] * 65)), {}, {}),
    "nres255_W4": (_nres_case(4, 255, 15, ring_base=1), {}, {}),
    "nres256_W4": (_nres_case(4, 256, 15, ring_base=1), {}, {}),
    "nres257_W4": (_nres_case(4, 257, 15, ring_base=1), {}, {}),
    "nres251_W4": (_nres_case(4, 251, 15, ring_base=1), {}, {}),
    "nres252_W4": (_nres_case(4, 252, 15, ring_base=1), {}, {}),
    "nres253_W4": (_nres_case(4, 253, 15, ring_base=1), {}, {}),
    "nres511_W4": (_nres_case(4, 511, 15, ring_base=1), {}, {}),
    "nres512_W4": (_nres_case(4, 512, 15, ring_base=1), {}, {}),
    "nres513_W4": (_nres_case(4, 513, 15, ring_base=1), {}, {}),
}
# Fa = 0, 1, 3, 4, 5, 16, 17 of F = 19 landmarks in the problem (fix_depth handles: lm_est_flag 1 = constant, 0 = variable)
for _fa in (0, 1, 3, 4, 5, 16, 17):
    CASES["Fa%d_W4" % _fa] = (dict(W=4, F0=17, seed=16, ring_base=3, rot_pre=2), dict(fix_depth=1), dict(n_var=_fa))
# a landmark seen from two coincident frames: Hll = 1e-29, the diagonal clamp [1e-6, 1e32] is active for it
CASES["flat_W4"] = (dict(W=4, F0=6, seed=19, flat=1, ring_base=2), {}, {})
# a bounds-constrained solve: two variable landmarks carry the inverse-depth bound, one of them starts beyond it
CASES["bounded_W4"] = (dict(W=4, F0=8, seed=17, ring_base=2), {}, dict(bound=2))
# a step that raises the cost (found by reject_scan)
# (without a prior and without the IMU: beside their near-quadratic terms no perturbation of the depths makes the full step raise the cost)
CASES["reject_W4"] = (dict(W=4, F0=8, seed=18, ring_base=1, use_imu=0, prior=None), dict(use_imu=0), dict(reject=1))

# ... and a bounds-constrained one: its projected full step misses the Armijo condition, so the line search has to shorten it
CASES["bounded_reject_W4"] = (dict(W=4, F0=8, seed=22, ring_base=1, use_imu=0, prior=None), dict(use_imu=0), dict(bound=2, reject=1))

REJECT_SCALES = (2.0, 2.5, 3.0, 3.5, 4.0)     # log-normal perturbation scales of the landmark depths the generator scans for a rejected step
NO_INTERP = ("ex_td_slow_W4", "flat_W4")               # cases whose branch points |gn| and alpha |g| lie within a factor 4: no radius is a factor 2 from both
FWD_UNBOUNDED = ()                            # cases whose C N eps kappa exceeds 1e-3 (test_solve_ref_cpu pins the list; at most one in eight)


def cfg_kwargs(name):
    kw, ck, _ = CASES[name]
    return dict(dict(window_size=kw["W"], max_landmarks=256), **ck)


def _post(case, cfg, post, name):
    st = case["st"]
    if "v0_scale" in post:
        st["Vs"] = st["Vs"].copy()
        st["Vs"][0] *= post["v0_scale"] / np.linalg.norm(st["Vs"][0]) * 0.6
        case["X"]["sb"][0, :3] = st["Vs"][0]
    if "n_var" in post:
        pl = [int(s) for s in st["lm_order"] if D._in_problem(st, s, case["W"])]
        st["lm_est_flag"] = st["lm_est_flag"].copy()
        for s in pl:
            st["lm_est_flag"][s] = 1
        # the variable ones spread over the list: every other position first, the last one always (the last row of Hpl belongs to it)
        pick = ([len(pl) - 1] + list(range(0, len(pl) - 1, 2)) + list(range(1, len(pl) - 1, 2)))[:post["n_var"]]
        for q in pick:
            st["lm_est_flag"][pl[q]] = 0
    if "bound" in post:
        pl = [int(s) for s in st["lm_order"] if D._in_problem(st, s, case["W"])]
        st["lm_est_flag"], st["lm_depth"] = st["lm_est_flag"].copy(), st["lm_depth"].copy()
        st["lm_est_flag"][pl[1]] = 2
        st["lm_est_flag"][pl[3]] = 2
        st["lm_depth"][pl[1]] = 0.8 * float(cfg.depth_max) / 2.0      # 1 / depth = 1.25 ub: beyond the bound, projected at x0
    return case


_case_cache, _pb_cache, _lin_cache = {}, {}, {}


def reject_scan(case0, cfg):
    """the first of REJECT_SCALES whose perturbation of the landmark depths makes the full step (radius 1e4) raise the cost beyond rejection by a
    factor 2 (rho < 5e-4): (case, scale) or (None, None)"""
    for sc in REJECT_SCALES:
        case = dict(case0, st=dict(case0["st"]))
        rng = np.random.default_rng([int(100 * sc), 5])
        case["st"]["lm_depth"] = case0["st"]["lm_depth"] * np.exp(sc * rng.standard_normal(len(case0["st"]["lm_depth"])))
        pb = Problem(case, cfg)
        X, feat = pb.x0()
        lin = linearise(pb, X, feat)
        st = gn_system(pb, lin, scaling(pb, lin))
        d = dogleg(st, RADIUS0)
        Xc, cf, _, _, _ = candidate(pb, X, feat, st.s, d["y"])
        fc, _ = cost(pb, Xc, cf)
        rho = float((lin.cost - fc) / d["model_change"])
        if rho < 0.5 * MIN_REL_DECREASE:
            return case, sc
    return None, None


def get_case(name, cfg):
    if name not in _case_cache:
        kw, _, post = CASES[name]
        case = _post(D.make_case(cfg, **kw), cfg, post, name)
        if post.get("reject"):
            case, sc = reject_scan(case, cfg)
            assert case is not None, "no listed perturbation scale gives a rejected step"
            case["reject_scale"] = sc
        _case_cache[name] = case
    return _case_cache[name]


def get_problem(name, cfg):
    if name not in _pb_cache:
        _pb_cache[name] = Problem(get_case(name, cfg), cfg)
    return _pb_cache[name]


def lin_at(name, cfg, X, feat):
    """the linearisation of a case at a point, cached on the point's bits"""
    pb = get_problem(name, cfg)
    key = (name,) + _key(X["pose"], X["sb"], X["ex"], X["td"], feat)
    if key not in _lin_cache:
        lin = linearise(pb, X, feat)
        _lin_cache[key] = (lin, gn_system(pb, lin, scaling(pb, lin)))
    return _lin_cache[key]


def ratio(got, want, bound):
    """worst |got - want| / bound (inf where an error meets a zero bound)"""
    e = np.abs((np.asarray(got, np.float64).astype(L) - np.asarray(want, L)).astype(np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), e.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e == 0, 0.0, e / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    return float(np.max(q)) if q.size else 0.0
