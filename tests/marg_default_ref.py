"""The DEFAULT marginalisation (vio_config.marg_exact = 0; be_kernels.hip marg_body as be_marg_kernel, be_marg_hbm_kernel and the be_marg_pre_kernel +
be_marg_alg_kernel pair run it) by its definition, on generated window states, with the error bounds of tests/test_gpu_marg_default.py.
tests/test_marg_default_ref_cpu.py checks this module against itself without a GPU.  Built from factor_ref (the factors, 40-digit mpmath) and
marg_ref (pseudo-inverse, gamma, C), not from the oracle and not from the device code's order of summation.

Parameters.  q = [m-block (md) | kept (n = 6 W + 16)].  MARGIN_OLD: md = 15 = pose 0 (6), speed-bias 0 (9); kept = pose 1 .. W in slots 0 .. W-1 (6 each),
speed-bias 1 (9), extrinsic (6), td (1); plus one inverse depth per landmark that is in the problem (!dyn, nobs >= 2, start < W - 2) and starts in
frame 0.  MARGIN_SECOND_NEW: md = 6 = pose W-1, kept = pose 0 .. W-2 in their slots, slot W-1 (pose W, which nothing touches), speed-bias 0, extrinsic,
td; only the prior contributes, and the stage does nothing at all unless the prior holds pose W-1.

Factors at the staged state (poses as (p, q) with q the quaternion of the staged rotation matrix, Eigen's conversion, formed in long double):
  prior       H, and the gradient r + H dx; dx by factor_ref.pose_delta against x0 for poses, plain differences for speed-bias and td, 0 where a block
              is absent.  The old prior's slots are pose 0 .. W-1, speed-bias 0, extrinsic, td.
  IMU (0, 1)  if use_imu and sum_dt < 10: G = [J r]^T C^-1 [J r] by factor_ref.gram_ref from the raw residual, the raw Jacobian (upstream's formulas)
              and the covariance of factor_ref.preint on the same samples.
  projection  every pair (0, k), k = 1 .. nobs - 1, of those landmarks, residual and Jacobian scaled by sqrt(rho') of CauchyLoss(1); the td column only
              with estimate_td, the extrinsic columns always.  inv_depth = fl(1 / depth), the parameter the device forms.
Reduction.  A = sum J^T J, b = sum J^T r.  Landmark l: c = J_q^T J_l, d = J_l^T J_l, b_l = J_l^T r; A -= c c^T / d, b -= c b_l / d where d > 1e-8, nothing
otherwise.  X = A_mm^+ with eigenvalues <= 1e-8 dropped (marg_ref.pinv_mp: mpmath at 40 digits, always -- the block is 15 x 15 at most).
A_r = A_rr - A_rm X A_mr, b_r = b_r0 - A_rm X b_m.  prior_H = sym(A_r), prior_r = b_r, c0 = b^T (sym(A_r) + delta I)^-1 b with
delta = 64 eps n max|diag A_r| (0 when the diagonal is zero).  prior_x0 = the kept parameters; the present mask = which factors touch which block.

Precision.  The factors come from factor_ref in mpmath, rounded to float64 (their rounding is part of the factor-level term below).  The sums, the
elimination, A_r, b_r and c0 run in 40-digit mpmath (numpy object arrays) for F0 <= 33 at W <= 4, in np.longdouble (64-bit mantissa) otherwise: the
object-array products cost 3 s (F0 = 17) to 6 s (F0 = 33) per W = 10 case against under 1 s, for 25 such cases in the CPU suite and again in the GPU
suite, and far more at W = 20.  The CPU test runs a W = 4 and a W = 10 case (F0 = 17, mq = 91) through both routes and finds them equal to 1e-17
relative to each entry's sum of absolute terms, four orders below the tightest bound here.

Bounds (eps = 2^-52, gamma_k = k eps / (1 - k eps), C = 8 as in marg_ref; KF = 64 is the factor-level constant tests/test_gpu_factor_edges.py holds
the device's factor routines to: a residual or Jacobian entry errs by at most KF eps scale, scale = factor_ref's cancellation-aware scale).
  reduced system over q (entrywise, EA / Eb):
      gamma_k (sum |J|^T |J| + sum |c| |c|^T / d + |H_prior| ...)      k = 2 residual rows + landmarks + 32: every entry of A is a sum of at most
                                                                      k products in some order, so gamma_k times the sum of absolute terms
    + sum (|dJ|^T |J| + |J|^T |dJ|)                                   first order in the factor-level error dJ = w KF eps scale_J + |w J| dw,
                                                                      dw = |r| . dr / (1 + |r|^2) + 4 eps the relative error of the Cauchy weight
    + (|dc| |c|^T + |c| |dc|^T) / d + |c| |c|^T dd / d^2              dc = |dJ_q|^T |J_l| + |J_q|^T |dJ_l| + gamma_2m |J_q|^T |J_l|, dd likewise
    + prior gradient: gamma_(n+1) (|r| + |H| |dx|) + |H| ddx          ddx = KF eps scale of pose_delta; the prior's H is copied, no error
    + IMU Gram: e_a sqrt(G_bb) + e_b sqrt(G_aa) + C (ns + 31) eps kappa(C) sqrt(G_aa G_bb)
      The device whitens with M = chol(cov)^-1 of ITS pre-integration.  A perturbation da of column a of [J r] moves G_ab by (M da) . (M b), at most
      |da|_2 / sqrt(lambda_min(C)) sqrt(G_bb) (Cauchy-Schwarz in the C^-1 inner product); e_a = C (ns + 1) KF eps |scale_a|_2 / sqrt(lambda_min(C)),
      both taken in the Jacobi scaling of C (scale_a over sqrt(diag C), lambda_min and kappa of diag(C)^-1/2 C diag(C)^-1/2: the Cholesky factor of the
      covariance is accurate relative to that),
      ns = samples (each step of the recursion adds a few eps of the running scale to dp / dq / dv / jac, which enter the columns linearly).  A
      relative perturbation t of C (recursion: (ns + 1) eps; Cholesky and the two 15-term products: 31 eps) moves C^-1 by at most kappa(C) t
      relatively, in the same inner product.
  A_r, b_r (entrywise): first order through A_rr - A_rm X A_mr with T = |A_rm| |X|:
      E_rr + E_rm |X| |A_mr| + T E_mr + T E_mm T^T + bx rn cn^T + gamma_(md+1) (|A_rr| + 2 T |A_mr|),   bx = C md eps |A~|_2 / lambda_min(A~)^2
      (marg_ref's bound of the pseudo-inverse, on the Jacobi-scaled block A~ = D A_mm D, D = diag(A_mm)^-1/2 over its non-zero rows: the block mixes
      entries of 1e5 (velocity) and 2e10 (gyroscope bias), and both a Cholesky inverse and a Jacobi eigen-decomposition of a positive definite
      matrix are accurate relative to the scaled matrix (Demmel, Veselic); rn / cn are the norms of the rows of A_rm D / columns of D A_mr).
      Valid while |D E_mm D|_2 <= 1e-3 lambda_min(A~) and the dropped eigenvalues are exact zeros of exactly zero rows (which the device
      reproduces exactly: nothing is ever added there); `bounded` says so.
  prior_H: sym(E_Ar) + eps |H|.   prior_r: E_br.
  c0: with M = sym(A_r) + delta I, y = M^-1 b, s = sqrt(diag M):  2 |y| . E_b + |y|^T E_H |y| + C n eps (|y| . s)^2 + gamma_n c0, over 1 - rho,
      rho = |D E_H D + C n eps 1 1^T|_2 |(D M D)^-1|_2 with D = diag(M)^-1/2 (c0 does not change under the scaling): the forward error of a backward
      stable Cholesky solve of the lifted matrix, whose backward error is componentwise |dM| <= gamma_(n+1) |L| |L^T| <= C n eps s s^T.  Where
      rho >= 1/2 the lifted matrix is singular to within its own error (a first marginalisation without a prior has the gauge directions in it) and
      c0 has no bound against the REFERENCE's value: `c0_bounded` is False (14 cases, by name in the CPU test).  Every case is also compared with
      c0 formed in mpmath from the returned prior_H and prior_r (`c0_self`, bound derived there), which holds the lift and the Cholesky solve
      to their own forward error whatever the error of H; only the six first marginalisations without a prior stay out (C0_UNDETERMINED).
Worst measured error / bound of float64 numpy and of the device: DESIGN.md section 5a.
"""

import mpmath
import numpy as np

import factor_ref as fr
import marg_ref as mr

L = np.longdouble
EPS = mr.EPS
C = mr.C
CUT = mr.CUT
KF = 64.0
gamma = mr.gamma
SLOTS = 200            # landmark slots a generated state uses (every handle of the tests has at least as many)
CAP = 64               # IMU samples per interval (VIO_IMU_SLOT_CAP)


# ------------------------------------------------------------------------------------------------------------ small helpers
def _qmul(a, b):   # (x y z w)
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _rotmat(q):
    """float64 rotation matrix of the unit quaternion (x y z w), formed in mpmath and rounded: what a test stages as Rs / ric"""
    with mpmath.workdps(fr.DPS):
        qq = [mpmath.mpf(float(x)) for x in (q[3], q[0], q[1], q[2])]
        nn = mpmath.sqrt(sum(x * x for x in qq))
        return np.array([[float(x) for x in r] for r in fr.q2R(tuple(x / nn for x in qq))])


def quat_of(R):
    """Eigen's Quaternion(Matrix3) on a float64 matrix with positive trace, in long double, rounded: (x y z w)"""
    R = np.asarray(R, np.float64).reshape(3, 3).astype(L)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    assert t > 0.01, "the generated rotations keep a positive trace"
    s = np.sqrt(t + 1)
    h = L(0.5) / s
    return np.array([(R[2, 1] - R[1, 2]) * h, (R[0, 2] - R[2, 0]) * h, (R[1, 0] - R[0, 1]) * h, L(0.5) * s]).astype(np.float64)


def to_mp_ld(M):
    """np.longdouble -> mpmath numbers, exactly (head and tail)"""
    M = np.asarray(M, L)
    out = np.empty(M.shape, object)
    for idx in np.ndindex(M.shape):
        hi = float(M[idx])
        out[idx] = mpmath.mpf(hi) + mpmath.mpf(float(M[idx] - L(hi)))
    return out


def _f64(M):
    M = np.asarray(M)
    if M.dtype == object:
        return np.array([float(x) for x in M.ravel()]).reshape(M.shape)
    return M.astype(np.float64)


def _as_ld(M):
    return mr.mp_to_ld(M) if np.asarray(M).dtype == object else np.asarray(M, L)


# ------------------------------------------------------------------------------------------------------------ the generator
DEFAULTS = dict(W=4, F0=5, seed=0, estimate_td=0, use_imu=1, prior="full", moved=0, second_new=0, flat=0, outlier=0, blind=0, long_dt=0, ring_base=0,
                rot_pre=0, shuffle=1, tr=0.0, extra_spec=())


def make_case(cfg, **kw):
    """A consistent pre-marginalisation state: smooth poses, landmarks with true geometry plus pixel noise, IMU samples, and a prior that is the
    positive semi-definite quadratic form of a smaller synthetic system.  cfg: the handle's Config (calibration and noise densities are read).
    kw (DEFAULTS): W, F0 = landmarks that are in the problem and start in frame 0; prior = None | "full" | "absent" (pose slots 1 and W-1, the
    extrinsic and td absent) | "no_pose_last" (pose W-1 absent: MARGIN_SECOND_NEW then does nothing); moved = 1: the state is off x0 by a few
    1e-2 in every present block and the quaternion of x0's pose 2 is negated (q0^-1 q has a negative scalar part); flat = the first `flat` of
    those landmarks are seen from frames 0 and 1 only, and frame 1 has the pose of frame 0 exactly (d = 0 up to round-off); outlier = 1: one
    observation is 0.2 off in x; blind = 1: no marginalised landmark sees frame W; long_dt = 1: interval 1 has sum_dt >= 10.
    extra_spec = further landmarks (start, nobs, dyn) behind the standard ones (tests/solve_ref.py: the solver's cases).
    Returns dict(kw, st = the tables for VioBatch.marg_stage_set in SLOTS slots (pad_tables widens them), X = the parameters)."""
    k = dict(DEFAULTS, **kw)
    W, F0 = k["W"], k["F0"]
    W1, n = W + 1, 6 * W + 16
    rng = np.random.default_rng([k["seed"], W, F0, 77])
    # ---- window: body moves along +x of the world with a little yaw / pitch; camera by the configuration's extrinsic
    ric = np.array(list(cfg.ric)).reshape(3, 3)
    tic = np.array(list(cfg.tic))
    Ps, Rs, Vs = np.zeros((W1, 3)), np.zeros((W1, 3, 3)), np.zeros((W1, 3))
    for i in range(W1):
        j = 0 if (k["flat"] and i == 1) else i
        th = np.array([0.01 * j, -0.015 * j, 0.03 * j + 0.002 * j * j])
        q = np.r_[0.5 * th, 1.0]
        Rs[i] = _rotmat(q / np.linalg.norm(q))
        Ps[i] = [0.12 * j + 0.004 * j * j, 0.03 * np.sin(0.7 * j), 0.01 * j]
        Vs[i] = [0.6 + 0.04 * j, 0.1 * np.cos(0.7 * j), 0.05]
    Bas = 0.02 * rng.standard_normal(3) + 1e-3 * rng.standard_normal((W1, 3))
    Bgs = 0.005 * rng.standard_normal(3) + 1e-4 * rng.standard_normal((W1, 3))
    dt_f = 0.2
    Headers = 100.0 + dt_f * np.arange(W1)
    td = 0.004 if k["estimate_td"] else float(cfg.td)
    g = np.array([0.0, 0.0, float(cfg.g_norm)])
    # ---- landmarks
    NLs = SLOTS
    lm = dict(lm_id=np.zeros(NLs, np.int32), lm_start=np.zeros(NLs, np.int32), lm_nobs=np.zeros(NLs, np.int32), lm_solve_flag=np.zeros(NLs, np.int32),
              lm_dyn=np.zeros(NLs, np.int32), lm_est_flag=np.zeros(NLs, np.int32), lm_depth=np.zeros(NLs), lm_obs=np.zeros((NLs, W1, 9)))
    top = W if k["blind"] else W1                          # frames a marginalised landmark may reach
    spec = []                                              # (start, nobs, dyn)
    for li in range(F0):
        lo = 3 if k["flat"] else 2                       # (frames 0 and 1 coincide in a flat case: a track of two would be flat as well)
        spec.append((0, 2 if li < k["flat"] else top if li % 3 == 2 else lo + (li + (li // 3)) % (top - lo + 1), 0))   # every third one reaches the last frame
    if F0 > k["flat"]:
        spec[F0 - 1] = (0, top, 0)                         # the longest track is always there
    spec += [(0, 3, 1), (1, min(3, W1 - 1), 0), (W - 2, 2, 0), (0, 1, 0), (1, W, 0)]       # dynamic, start > 0, start >= W - 2, nobs = 1, a long later one
    spec += [tuple(int(v) for v in e) for e in k["extra_spec"]]
    assert len(spec) <= NLs
    slots = rng.permutation(NLs)[:len(spec)] if k["shuffle"] else np.arange(len(spec))
    order = np.array(slots, np.int32)
    if k["shuffle"]:
        order = order[rng.permutation(len(order))]
    fx, fy, cx, cy = float(cfg.fx), float(cfg.fy), float(cfg.cx), float(cfg.cy)
    rb = k["ring_base"] % W1
    for (start, nobs, dyn), slot in zip(spec, slots):
        xy = rng.uniform(-0.45, 0.45, 2) * [1.0, 0.7]
        D = rng.uniform(2.0, 6.0)
        Rc0, Pc0 = Rs[start] @ ric, Ps[start] + Rs[start] @ tic
        pw = Rc0 @ (D * np.r_[xy, 1.0]) + Pc0
        for a in range(nobs):
            f = start + a
            Rc, Pc = Rs[f] @ ric, Ps[f] + Rs[f] @ tic
            pc = Rc.T @ (pw - Pc)
            x, y = pc[0] / pc[2] + rng.normal(0, 0.5 / fx), pc[1] / pc[2] + rng.normal(0, 0.5 / fy)
            if a == 0:
                x, y = xy
            vel = rng.normal(0, 0.05, 2)
            lm["lm_obs"][slot, (f + rb) % W1] = [x, y, 1.0, fx * x + cx, fy * y + cy, vel[0], vel[1], float(cfg.td), pc[2]]
        lm["lm_id"][slot] = 1000 + slot
        lm["lm_start"][slot], lm["lm_nobs"][slot], lm["lm_dyn"][slot] = start, nobs, dyn
        lm["lm_solve_flag"][slot], lm["lm_est_flag"][slot] = 1, 1
        lm["lm_depth"][slot] = D * (1.0 + 0.01 * rng.standard_normal())
    if k["outlier"] and F0 > k["flat"]:
        slot = slots[F0 - 1]
        lm["lm_obs"][slot, (1 + rb) % W1, 0] += 0.2
    # ---- IMU: samples of every interval, consistent with the motion only loosely (the residual is whatever it is)
    imu = dict(imu_n=np.zeros(W1, np.int32), imu_dt=np.zeros((W1, CAP)), imu_acc=np.zeros((W1, CAP, 3)), imu_gyr=np.zeros((W1, CAP, 3)),
               imu_acc0=np.zeros((W1, 3)), imu_gyr0=np.zeros((W1, 3)), imu_ba=np.zeros((W1, 3)), imu_bg=np.zeros((W1, 3)))
    for j in range(1, W1):
        ns = 60 if (k["long_dt"] and j == 1) else 7 + (j % 3)
        h = 0.2 if (k["long_dt"] and j == 1) else dt_f / ns
        imu["imu_n"][j] = ns
        imu["imu_dt"][j, :ns] = h * (1.0 + 0.01 * rng.standard_normal(ns))
        imu["imu_acc"][j, :ns] = Rs[j].T @ g + [0.4, 0.1, 0.0] + 0.05 * rng.standard_normal((ns, 3))
        imu["imu_gyr"][j, :ns] = [0.05, -0.07, 0.15] + 0.01 * rng.standard_normal((ns, 3))
        imu["imu_acc0"][j], imu["imu_gyr0"][j] = imu["imu_acc"][j, 0] + 0.01, imu["imu_gyr"][j, 0] - 0.002
        imu["imu_ba"][j], imu["imu_bg"][j] = Bas[j - 1] + 2e-3 * rng.standard_normal(3), Bgs[j - 1] + 2e-4 * rng.standard_normal(3)
    pre_idx = np.roll(np.arange(W1, dtype=np.int32), k["rot_pre"])
    # ---- parameters
    pose = np.zeros((W1, 7))
    for i in range(W1):
        pose[i] = np.r_[Ps[i], quat_of(Rs[i])]
    sb = np.hstack([Vs, Bas, Bgs])
    ex = np.r_[tic, quat_of(_rotmat_of(ric))]
    ric_s = _rotmat_of(ric)
    X = dict(pose=pose, sb=sb, ex=ex, td=td)
    # ---- prior
    prior = None
    if k["prior"]:
        present = np.ones(W + 3, np.int32)
        if k["prior"] == "absent":
            present[[1, W + 1, W + 2] if k["second_new"] else [1, W - 1, W + 1, W + 2]] = 0
        if k["prior"] == "no_pose_last":
            present[W - 1] = 0
        if not k["estimate_td"]:
            present[W + 2] = 0
        mask = np.concatenate([np.repeat(present[:W], 6), np.repeat(present[W], 9), np.repeat(present[W + 1], 6), [present[W + 2]]]).astype(bool)
        rows = 2 * n
        G = rng.standard_normal((rows, n)) * np.concatenate([np.full(6 * W, 30.0), np.full(3, 10.0), np.full(6, 300.0), np.full(6, 100.0), [50.0]])
        G[:, ~mask] = 0.0
        e = rng.standard_normal(rows)
        H = G.T @ G
        H = 0.5 * (H + H.T)
        x0 = np.concatenate([pose[:W].ravel(), sb[0], ex, [td]])
        if k["moved"]:
            for s in range(W):
                d6 = 0.02 * rng.standard_normal(6)
                qd = np.r_[0.5 * d6[3:], 1.0]
                q0 = _qmul(pose[s, 3:], qd / np.linalg.norm(qd))
                x0[7 * s:7 * s + 7] = np.r_[pose[s, :3] + d6[:3], q0]
            x0[14:21][3:] *= -1.0                                    # pose 2 (present in every prior here): the same rotation, q0^-1 q with a negative scalar part
            x0[7 * W:7 * W + 9] += np.r_[0.02 * rng.standard_normal(3), 1e-3 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)]
            qd = np.r_[0.005 * rng.standard_normal(3), 1.0]
            x0[7 * W + 9:7 * W + 16] = np.r_[ex[:3] + 0.01 * rng.standard_normal(3), _qmul(ex[3:], qd / np.linalg.norm(qd))]
            x0[7 * W + 16] += 1e-3
        prior = dict(present=present, H=H, r=G.T @ e, x0=x0)
    st = dict(lm, lm_order=order, Ps=Ps, Rs=Rs, Headers=Headers, ric=ric_s, tic=tic, Vs=Vs, Bas=Bas, Bgs=Bgs, g=g, td=td, ring_base=rb,
              marginalization_flag=int(k["second_new"]), pre_idx=pre_idx, prior=prior)
    if k["use_imu"]:
        st.update(imu)
    return dict(k, st=st, X=X, F0_spec=F0)


def _rotmat_of(R):
    """the staged extrinsic rotation: the configuration's matrix, re-orthonormalised through its quaternion as the library does on creation"""
    return _rotmat(quat_of(R))


def pad_tables(st, NL):
    """the tables widened from SLOTS to a handle's NL slots"""
    out = dict(st)
    for name in ("lm_id", "lm_start", "lm_nobs", "lm_solve_flag", "lm_dyn", "lm_est_flag", "lm_depth", "lm_obs"):
        a = np.asarray(st[name])
        assert NL >= a.shape[0]
        z = np.zeros((NL,) + a.shape[1:], a.dtype)
        z[:a.shape[0]] = a
        out[name] = z
    return out


# ------------------------------------------------------------------------------------------------------------ the factors, with their error terms
def prior_dx(X, x0, present, W, cv):
    """The prior's tangent dx = x (-) x0 over its n = 6 W + 16 slots (pose 0 .. W-1, speed-bias 0, extrinsic, td; 0 where a block is absent), the
    scale of each entry's error (ddx = KF eps scale) and the smallest scalar part of q0^-1 q met"""
    n = 6 * W + 16
    dx, sdx, w_min = np.zeros(n), np.zeros(n), None
    for s in range(W):
        if present[s]:
            d6, s6, w = fr.pose_delta(X["pose"][s], x0[7 * s:7 * s + 7])
            dx[6 * s:6 * s + 6], sdx[6 * s:6 * s + 6] = d6, s6
            w_min = float(w) if w_min is None else min(w_min, float(w))
    if present[W]:
        dx[6 * W:6 * W + 9] = _f64(cv(X["sb"][0]) - cv(x0[7 * W:7 * W + 9]))
        sdx[6 * W:6 * W + 9] = np.maximum(np.abs(X["sb"][0]), np.abs(x0[7 * W:7 * W + 9]))
    if present[W + 1]:
        d6, s6, _ = fr.pose_delta(X["ex"], x0[7 * W + 9:7 * W + 16])
        dx[6 * W + 9:6 * W + 15], sdx[6 * W + 9:6 * W + 15] = d6, s6
    if present[W + 2]:
        dx[6 * W + 15] = X["td"] - x0[7 * W + 16]
        sdx[6 * W + 15] = max(abs(X["td"]), abs(x0[7 * W + 16]))
    return dx, sdx, w_min


_pre_cache = {}


def imu_pre(cfg, st, j):
    """factor_ref.preint of the samples of the interval that ends in frame j (cached on the samples)"""
    ns = int(st["imu_n"][j])
    noise = (float(cfg.acc_n), float(cfg.gyr_n), float(cfg.acc_w), float(cfg.gyr_w))
    a = (st["imu_dt"][j, :ns], st["imu_acc"][j, :ns], st["imu_gyr"][j, :ns], st["imu_acc0"][j], st["imu_gyr0"][j], st["imu_ba"][j], st["imu_bg"][j])
    key = tuple(np.ascontiguousarray(x, np.float64).tobytes() for x in a) + (noise,)
    if key not in _pre_cache:
        _pre_cache[key] = fr.preint(*a, noise)
    return _pre_cache[key], ns


def imu_gram(cfg, pre, ns, pi, sbi, pj, sbj):
    """The IMU factor between two frames at the given parameters: G = [J r]^T C^-1 [J r] (31 x 31, columns pose_i, speed-bias_i, pose_j,
    speed-bias_j, residual), its entrywise error bound EG (module docstring) and kappa of the Jacobi-scaled covariance"""
    a4 = (pre, float(cfg.g_norm), pi, sbi, pj, sbj)
    rr, rs = fr.imu_residual(*a4)
    Jf, Js = fr.imu_jacobian_formula(*a4)
    rs = np.maximum(rs, np.r_[np.full(3, pre["scale_p"]), np.ones(3), np.full(3, pre["scale_v"]), np.zeros(6)])
    G = fr.gram_ref(Jf, rr, pre["cov"])
    cov = 0.5 * (pre["cov"] + pre["cov"].T)
    dc_ = 1.0 / np.sqrt(np.diag(cov))
    ev = np.linalg.eigvalsh(cov * np.outer(dc_, dc_))          # the Jacobi-scaled covariance: what a Cholesky factor's accuracy depends on
    kappa = float(ev[-1] / ev[0])
    cols = np.hstack([Js, rs[:, None]]) * dc_[:, None]
    e_col = C * (ns + 1) * KF * EPS * np.sqrt((cols * cols).sum(axis=0)) / np.sqrt(ev[0])
    sg = np.sqrt(np.abs(np.diag(G)))
    EG = e_col[:, None] * sg[None, :] + sg[:, None] * e_col[None, :] + C * (ns + 31) * EPS * kappa * np.outer(sg, sg)
    return G, EG, kappa


def proj_rows(K, pi, pj, ex, inv_dep, td, oi, oj, use_td):
    """One projection pair under CauchyLoss(1): the weighted Jacobian w J (2 x 20: pose_i, pose_j, extrinsic, td, inverse depth), the weighted
    residual w r, their factor-level error bounds dJ, dr (module docstring), the weight w = sqrt(rho') and the raw residual"""
    a9 = (K, pi, pj, ex, inv_dep, td, oi, oj, use_td)
    r2, r2s = fr.proj_residual(*a9)
    J, Js = fr.proj_jacobian_formula(*a9)
    w = fr.cauchy_weight(r2)
    dw = float(np.abs(r2) @ (KF * EPS * r2s)) / (1.0 + float(r2 @ r2)) + 4 * EPS
    return w * J, w * KF * EPS * Js + np.abs(w * J) * dw, w * r2, w * KF * EPS * r2s + np.abs(w * r2) * dw, w, r2, r2s


# ------------------------------------------------------------------------------------------------------------ the definition
class Ref:
    pass


def _in_problem(st, slot, W):
    return (not st["lm_dyn"][slot]) and st["lm_nobs"][slot] >= 2 and st["lm_start"][slot] < W - 2


def marg_list(case):
    """slots of the landmarks the marginalisation eliminates, in list order"""
    st, W = case["st"], case["W"]
    n_lm = len(st["lm_order"])
    return [int(s) for s in st["lm_order"][:n_lm] if _in_problem(st, s, W) and st["lm_start"][s] == 0]


def reference(case, cfg, route=None):
    """The definition on one case.  route: "mp" | "ld" | None (mp for F0 <= 33 at W <= 4)."""
    st, X, W = case["st"], case["X"], case["W"]
    n, W1 = 6 * W + 16, W + 1
    second_new = bool(st["marginalization_flag"])
    prior = st["prior"]
    r = Ref()
    r.W, r.n, r.second_new = W, n, second_new
    r.has_prior_in = prior is not None
    present_in = np.array(prior["present"] if prior is not None else np.zeros(W + 3), np.int32)
    if second_new and not (prior is not None and present_in[W - 1]):
        r.noop = True                                   # estimator.cpp: MARGIN_SECOND_NEW marginalises only when the prior holds pose W-1
        r.present, r.has_prior = present_in, int(prior is not None)
        return r
    r.noop = False
    lst = marg_list(case) if not second_new else []
    r.list = lst
    route = route or ("mp" if (len(lst) <= 33 and W <= 4) else "ld")
    r.route = route
    cv = mr.to_mp if route == "mp" else (lambda a: np.asarray(a, np.float64).astype(L))
    md = 6 if second_new else 15
    mq = md + n
    r.md, r.mq = md, mq
    rS, rE, rT = md + 6 * W, md + 6 * W + 9, md + 6 * W + 15
    like = cv(np.zeros(1))
    A, b = mr._zeros((mq, mq), like), mr._zeros(mq, like)
    absA, absb = np.zeros((mq, mq)), np.zeros(mq)          # sums of absolute terms
    EA, Eb = np.zeros((mq, mq)), np.zeros(mq)              # first-order factor-level error
    terms = 32
    present = np.zeros(W + 3, np.int32)
    # ---- prior
    if prior is not None:
        def pm(a):
            if a < 6 * W:
                kk, d = divmod(a, 6)
                if second_new:
                    return d if kk == W - 1 else md + 6 * kk + d
                return d if kk == 0 else md + 6 * (kk - 1) + d
            if a < 6 * W + 9:
                return (rS if second_new else 6) + (a - 6 * W)
            if a < 6 * W + 15:
                return rE + (a - 6 * W - 9)
            return rT
        idx = np.array([pm(a) for a in range(n)])
        H, pr, x0 = np.asarray(prior["H"], np.float64), np.asarray(prior["r"], np.float64), np.asarray(prior["x0"], np.float64)
        dx, sdx, r.w_min = prior_dx(X, x0, present_in, W, cv)
        r.dx, r.prior_idx = dx, idx
        Hc = cv(H)
        grad = cv(pr) + Hc @ cv(dx)
        A[np.ix_(idx, idx)] = A[np.ix_(idx, idx)] + Hc
        b[idx] = b[idx] + grad
        absA[np.ix_(idx, idx)] += np.abs(H)
        absb[idx] += np.abs(pr) + np.abs(H) @ np.abs(dx)
        Eb[idx] += gamma(n + 1) * (np.abs(pr) + np.abs(H) @ np.abs(dx)) + np.abs(H) @ (KF * EPS * sdx)
        if second_new:
            present[:W - 1] = present_in[:W - 1]
            present[W], present[W + 1], present[W + 2] = present_in[W], present_in[W + 1], present_in[W + 2]
        else:
            present[:W - 1] = present_in[1:W]
            present[W + 1], present[W + 2] = present_in[W + 1], present_in[W + 2]
    K = fr.proj_consts(cfg)
    use_td = bool(cfg.estimate_td)
    r.imu_used = False
    r.d, r.d_err, r.weights = [], [], []
    if not second_new:
        # ---- IMU factor (0, 1)
        if cfg.use_imu:
            j = 1
            pre, ns = imu_pre(cfg, st, j)
            r.sum_dt = pre["sum_dt"]
            if pre["sum_dt"] < 10.0:
                r.imu_used = True
                G, EG, r.cov_kappa = imu_gram(cfg, pre, ns, X["pose"][0], X["sb"][0], X["pose"][1], X["sb"][1])
                ii = np.r_[np.arange(15), md + np.arange(6), rS + np.arange(9)]
                Gc = cv(G)
                A[np.ix_(ii, ii)] = A[np.ix_(ii, ii)] + Gc[:30, :30]
                b[ii] = b[ii] + Gc[:30, 30]
                absA[np.ix_(ii, ii)] += np.abs(G[:30, :30])
                absb[ii] += np.abs(G[:30, 30])
                EA[np.ix_(ii, ii)] += EG[:30, :30]
                Eb[ii] += EG[:30, 30]
                present[0], present[W] = 1, 1
        # ---- projection factors of the landmarks that start in frame 0
        rb = int(st["ring_base"])
        for slot in lst:
            no = int(st["lm_nobs"][slot])
            m = no - 1
            inv_dep = 1.0 / float(st["lm_depth"][slot])
            oi = st["lm_obs"][slot, (0 + rb) % W1]
            Jq, Jl, rw = np.zeros((2 * m, mq)), np.zeros(2 * m), np.zeros(2 * m)
            dJq, dJl, drw = np.zeros((2 * m, mq)), np.zeros(2 * m), np.zeros(2 * m)
            for kf in range(1, no):
                oj = st["lm_obs"][slot, (kf + rb) % W1]
                wJ, dJ, wr, dr, w, _, _ = proj_rows(K, X["pose"][0], X["pose"][kf], X["ex"], inv_dep, X["td"], oi, oj, use_td)
                r.weights.append(w)
                cols = np.r_[np.arange(6), md + 6 * (kf - 1) + np.arange(6), rE + np.arange(6)]
                src = np.arange(18)
                if use_td:
                    cols, src = np.r_[cols, rT], np.arange(19)
                rows = slice(2 * (kf - 1), 2 * kf)
                Jq[rows, cols] = wJ[:, src]
                dJq[rows, cols] = dJ[:, src]
                Jl[rows], dJl[rows] = wJ[:, 19], dJ[:, 19]
                rw[rows], drw[rows] = wr, dr
                present[kf - 1] = 1
            present[W + 1] = 1
            if use_td:
                present[W + 2] = 1
            cc = np.flatnonzero(np.any(Jq != 0, axis=0) | np.any(dJq != 0, axis=0))
            Jc, Jlc, rc = cv(Jq[:, cc]), cv(Jl), cv(rw)
            aJ, adJ = np.abs(Jq[:, cc]), dJq[:, cc]
            A[np.ix_(cc, cc)] = A[np.ix_(cc, cc)] + Jc.T @ Jc
            b[cc] = b[cc] + Jc.T @ rc
            absA[np.ix_(cc, cc)] += aJ.T @ aJ
            absb[cc] += aJ.T @ np.abs(rw)
            EA[np.ix_(cc, cc)] += adJ.T @ aJ + aJ.T @ adJ
            Eb[cc] += adJ.T @ np.abs(rw) + aJ.T @ drw
            c, d, bl = Jc.T @ Jlc, Jlc @ Jlc, Jlc @ rc
            g2 = gamma(2 * m)
            ac, ad, abl = aJ.T @ np.abs(Jl), float(np.abs(Jl) @ np.abs(Jl)), float(np.abs(Jl) @ np.abs(rw))
            dc = adJ.T @ np.abs(Jl) + aJ.T @ dJl + g2 * ac
            dd = 2 * float(np.abs(Jl) @ dJl) + g2 * ad
            dbl = float(dJl @ np.abs(rw) + np.abs(Jl) @ drw) + g2 * abl
            r.d.append(float(d))
            r.d_err.append(dd)
            terms += 2 * m + 1
            if d > CUT:
                A[np.ix_(cc, cc)] = A[np.ix_(cc, cc)] - np.outer(c, c) / d
                b[cc] = b[cc] - c * (bl / d)
                fc, fd, fbl = np.abs(_f64(c)), float(d), abs(float(bl))
                absA[np.ix_(cc, cc)] += np.outer(fc, fc) / fd
                absb[cc] += fc * fbl / fd
                EA[np.ix_(cc, cc)] += (np.outer(dc, fc) + np.outer(fc, dc)) / fd + np.outer(fc, fc) * dd / fd ** 2
                Eb[cc] += (dc * fbl + fc * dbl) / fd + fc * fbl * dd / fd ** 2
    r.terms = terms
    r.A, r.b = _as_ld(A), _as_ld(b)
    r.EA = EA + gamma(terms) * absA
    r.Eb = Eb + gamma(terms) * absb
    r.absA, r.absb = absA, absb
    r.present, r.has_prior = present, 1
    # ---- the m-block
    Amm = r.A[:md, :md]
    r.zero_rows = np.flatnonzero(~np.any(_f64(Amm) != 0, axis=1))
    with mpmath.workdps(mr.R.DPS):
        Xo, kept, dropped = _pinv_mp(A[:md, :md] if route == "mp" else to_mp_ld(Amm))
    r.lam_kept_min = min(kept) if kept else None
    r.lam_drop_max = max(dropped) if dropped else None
    r.n_dropped = len(dropped)
    Xl = mr.mp_to_ld(Xo)
    r.X = Xl
    Arm, Amr, Arr = r.A[md:, :md], r.A[:md, md:], r.A[md:, md:]
    bm, br0 = r.b[:md], r.b[md:]
    if route == "mp":
        Am, bmp = A, b
        T1 = Am[md:, :md] @ Xo
        Ar, br = Am[md:, md:] - T1 @ Am[:md, md:], bmp[md:] - T1 @ bmp[:md]
        r.Ar, r.br = mr.mp_to_ld(Ar), mr.mp_to_ld(br)
    else:
        T1 = Arm @ Xl
        r.Ar, r.br = Arr - T1 @ Amr, br0 - T1 @ bm
    # the block Jacobi-scaled over its non-zero rows: Cholesky and Jacobi are accurate relative to D A_mm D, D = diag(A_mm)^-1/2
    Af = _f64(Amm)
    nz = np.flatnonzero(np.any(Af != 0, axis=1))
    Dm = np.zeros(md)
    Dm[nz] = 1.0 / np.sqrt(np.diag(Af)[nz])
    As = Af * np.outer(Dm, Dm)
    evs = np.linalg.eigvalsh(0.5 * (As[np.ix_(nz, nz)] + As[np.ix_(nz, nz)].T)) if len(nz) else np.zeros(0)
    r.scaled_lmin, r.scaled_norm = (float(evs[0]), float(evs[-1])) if len(nz) else (None, 0.0)
    bx = C * md * EPS * r.scaled_norm / r.scaled_lmin ** 2 if len(nz) else 0.0
    aX = np.abs(_f64(Xl))
    aArm, aAmr = np.abs(_f64(Arm)), np.abs(_f64(Amr))
    T = aArm @ aX
    Emm, Emr, Erm, Err = r.EA[:md, :md], r.EA[:md, md:], r.EA[md:, :md], r.EA[md:, md:]
    rn, cn = np.sqrt(((aArm * Dm[None, :]) ** 2).sum(axis=1)), np.sqrt(((aAmr * Dm[:, None]) ** 2).sum(axis=0))
    g = gamma(md + 1)
    r.Ar_bound = Err + Erm @ (aX @ aAmr) + T @ Emr + T @ Emm @ T.T + bx * np.outer(rn, cn) + g * (np.abs(_f64(Arr)) + 2 * T @ aAmr)
    abm = np.abs(_f64(bm))
    r.br_bound = (r.Eb[md:] + Erm @ (aX @ abm) + T @ r.Eb[:md] + T @ Emm @ (aX @ abm) + bx * rn * float(np.linalg.norm(abm * Dm)) +
                  g * (np.abs(_f64(br0)) + 2 * T @ abm))
    # the first-order propagation holds while the block's (scaled) error is far below its smallest kept (scaled) eigenvalue, and what is dropped
    # is exactly zero
    zr = r.zero_rows
    r.rho_mm = mr.norm2(Emm * np.outer(Dm, Dm)) / r.scaled_lmin if len(nz) else 0.0
    r.bounded = bool(r.rho_mm <= 1e-3 and len(zr) == r.n_dropped and not Emm[zr].any() and
                     (not dropped or max(abs(x) for x in dropped) <= 1e-25 * max(mr.norm2(Af), 1.0)))
    # ---- the new prior
    r.H = 0.5 * (r.Ar + r.Ar.T)
    Hf = _f64(r.H)
    r.H_bound = 0.5 * (r.Ar_bound + r.Ar_bound.T) + EPS * np.abs(Hf)
    r.r_bound = r.br_bound
    dmax = float(np.max(np.abs(np.diag(Hf)))) if n else 0.0
    r.delta = 64.0 * EPS * n * dmax
    r.c0, r.c0_bound, r.c0_bounded = L(0), 0.0, True
    if dmax > 0:
        M = r.H + L(r.delta) * np.eye(n, dtype=L)
        Mi = mr.gauss_inverse(M)
        y = Mi @ r.br
        r.c0 = r.br @ y
        ay = np.abs(_f64(y))
        sd = np.sqrt(np.diag(_f64(M)))
        Dg = 1.0 / sd
        Es = r.H_bound * np.outer(Dg, Dg) + C * n * EPS * np.ones((n, n))
        Ms = _f64(M) * np.outer(Dg, Dg)
        lmin = float(np.linalg.eigvalsh(0.5 * (Ms + Ms.T))[0])
        rho = mr.norm2(Es) / lmin if lmin > 0 else np.inf
        r.rho = float(rho)
        r.c0_bounded = bool(rho < 0.5)
        first = 2 * float(ay @ r.r_bound) + float(ay @ r.H_bound @ ay) + C * n * EPS * float(ay @ sd) ** 2 + gamma(n) * abs(float(r.c0))
        r.c0_bound = first / (1 - rho) if r.c0_bounded else np.inf
    # ---- prior_x0: the kept parameters, shifted
    x0n = np.zeros(7 * W + 17)
    for t in range(W):
        src = (W if t == W - 1 else t) if second_new else t + 1
        x0n[7 * t:7 * t + 7] = X["pose"][src]
    x0n[7 * W:7 * W + 9] = X["sb"][0 if second_new else 1]
    x0n[7 * W + 9:7 * W + 16] = X["ex"]
    x0n[7 * W + 16] = X["td"]
    r.x0 = x0n
    r.x0_quat = np.zeros(7 * W + 17, bool)                 # entries that pass through the device's matrix -> quaternion conversion
    for t in list(range(W)):
        r.x0_quat[7 * t + 3:7 * t + 7] = True
    r.x0_quat[7 * W + 12:7 * W + 16] = True
    return r


def _pinv_mp(Amm):
    """marg_ref.pinv_mp on a matrix that already holds mpmath numbers"""
    m = Amm.shape[0]
    E, Q = mpmath.eigsy(mpmath.matrix(Amm.tolist()))
    D = mpmath.matrix(m, m)
    for k in range(m):
        D[k, k] = 1 / E[k] if E[k] > CUT else 0
    Xm = Q * D * Q.T
    Xo = np.empty((m, m), object)
    for i in range(m):
        for j in range(m):
            Xo[i, j] = Xm[i, j]
    ev = [E[k] for k in range(m)]
    return Xo, [float(e) for e in ev if e > CUT], [float(e) for e in ev if not e > CUT]


# ------------------------------------------------------------------------------------------------------------ float64 numpy on the same inputs
def np_eval(ref, A=None, b=None):
    """The reduction in float64 numpy from the reference's reduced system rounded to float64 (or from A, b given instead): A_r, b_r, H, c0
    (numpy.linalg.eigh for the pseudo-inverse, numpy.linalg.cholesky for c0)."""
    md = ref.md
    A, b = _f64(ref.A if A is None else A), _f64(ref.b if b is None else b)
    w, V = np.linalg.eigh(0.5 * (A[:md, :md] + A[:md, :md].T))
    Xf = (V * np.where(w > CUT, 1.0 / np.where(w > CUT, w, 1.0), 0.0)) @ V.T
    T1 = A[md:, :md] @ Xf
    Ar, br = A[md:, md:] - T1 @ A[:md, md:], b[md:] - T1 @ b[:md]
    H = 0.5 * (Ar + Ar.T)
    c0 = 0.0
    dmax = np.abs(np.diag(Ar)).max()
    if dmax > 0:
        try:
            Lc = np.linalg.cholesky(H + 64.0 * EPS * ref.n * dmax * np.eye(ref.n))
            z = np.linalg.solve(Lc, br)
            c0 = float(z @ z)
        except np.linalg.LinAlgError:
            c0 = 0.0
    return Ar, br, H, c0


_self_cache = {}


def c0_self(H, rr):
    """c0 by its definition from a RETURNED prior: b^T (H + delta I)^-1 b, delta = 64 eps n max|diag H|, in 40-digit mpmath on the float64 (H, b) as
    given -- what the kernel's Cholesky solve is asked to compute, whatever the error of H itself.  Returns (c0, bound, rho, pd).
    With D = diag(M)^-1/2, M~ = D M D (unit diagonal), b~ = D b, y~ = M~^-1 b~: a backward-stable Cholesky solve returns b~^T (M~ + E)^-1 b~ with
    |E|_2 <= C n eps |M~|_2 (marg_ref's convention for a backward-stable solver; the factorisation is invariant under the scaling), so
    |dc0| <= (C n eps |M~|_2 |y~|_2^2 + gamma_n c0) / (1 - rho), rho = C n eps |M~|_2 / lambda_min(M~), and with rho < 1/2 the factorisation cannot
    break down.  lambda_min(M~) is numpy.linalg.eigvalsh's less its own error n eps |M~|_2.  pd: M~ has a Cholesky factor in mpmath.  Where pd is
    False or rho >= 1/2 the lifted matrix of this H is not positive definite to within the solve's own backward error: neither the value nor
    whether the factorisation succeeds is determined (the kernel returns 0 when it breaks down)."""
    H, rr = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(rr, np.float64)
    key = (H.tobytes(), rr.tobytes())
    if key in _self_cache:
        return _self_cache[key]
    n = len(rr)
    dmax = float(np.abs(np.diag(H)).max())
    if not dmax > 0:
        out = (0.0, 0.0, 0.0, True)
    else:
        with mpmath.workdps(fr.DPS):
            M = mr.to_mp(0.5 * (H + H.T))          # (H is returned exactly symmetric: the mean is exact)
            dl = mpmath.mpf(64.0 * EPS * n * dmax)
            for i in range(n):
                M[i, i] = M[i, i] + dl
            s = [mpmath.sqrt(M[i, i]) for i in range(n)]
            Ms = mpmath.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    Ms[i, j] = M[i, j] / (s[i] * s[j])
            bs = mpmath.matrix([mpmath.mpf(float(rr[i])) / s[i] for i in range(n)])
            try:
                y, pd = mpmath.cholesky_solve(Ms, bs), True
            except (ValueError, ZeroDivisionError):
                y, pd = mpmath.lu_solve(Ms, bs), False
            c0 = float(sum(bs[i] * y[i] for i in range(n)))
            y2 = float(sum(y[i] * y[i] for i in range(n)))
            Mf = np.array([[float(Ms[i, j]) for j in range(n)] for i in range(n)])
        w = np.linalg.eigvalsh(Mf)
        nM = float(w[-1])
        lmin = float(w[0]) - n * EPS * nM
        E = C * n * EPS * nM
        rho = E / lmin if lmin > 0 else np.inf
        bound = (E * y2 + gamma(n) * abs(c0)) / (1 - rho) if rho < 0.5 else np.inf
        out = (c0, bound, float(rho), pd)
    _self_cache[key] = out
    return out


def ratios(ref, H, rr, c0, A=None, b=None, Ar=None, br=None):
    """worst error / bound of a set of outputs: dict (inf where an error meets a zero bound)"""
    tiny = np.finfo(np.float64).tiny

    def rat(got, want, bound):
        e = np.abs((np.asarray(got, np.float64).astype(L) - want).astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0, 0.0, e / np.maximum(bound, tiny * (bound == 0)))
        return float(np.max(q)) if q.size else 0.0
    out = {"H": rat(H, ref.H, ref.H_bound), "r": rat(rr, ref.br, ref.r_bound)}
    if ref.c0_bounded:
        out["c0"] = rat(np.array([c0]), np.array([ref.c0], L), np.array([ref.c0_bound]))
    if A is not None:
        mq = ref.mq
        out["A"] = rat(np.asarray(A).reshape(-1)[:mq * mq].reshape(mq, mq), ref.A, ref.EA)
        out["b"] = rat(np.asarray(b)[:mq], ref.b, ref.Eb)
    if Ar is not None:
        out["A_r"] = rat(Ar, ref.Ar, ref.Ar_bound)
        out["b_r"] = rat(br, ref.br, ref.br_bound)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases of the GPU test
F0_LIST = [0, 1, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]

KINDS = {
    "td":          dict(estimate_td=1, tr=0.02, F0=17),
    "no_prior":    dict(prior=None, F0=17),
    "absent":      dict(prior="absent", F0=17),
    "moved":       dict(moved=1, F0=17, estimate_td=1, tr=0.02),
    "moved_absent": dict(moved=1, prior="absent", F0=5),
    "no_imu":      dict(use_imu=0, prior=None, F0=17),
    "long_dt":     dict(long_dt=1, prior=None, F0=17),
    "flat1":       dict(flat=1, F0=5),
    "flat3":       dict(flat=3, F0=17, outlier=1),
    "blind":       dict(blind=1, F0=17),
    "second_new":  dict(second_new=1, F0=5),
    "second_new_absent": dict(second_new=1, prior="absent", F0=5, moved=1),
    "second_new_noop": dict(second_new=1, prior="no_pose_last", F0=5),
    "second_new_no_prior": dict(second_new=1, prior=None, F0=5),
}


def case_list():
    """(name, W, kwargs): every F0 of F0_LIST at W = 4, the trips and tails again at W = 10, every kind at W = 4 and W = 10, and the wide windows
    (W = 12, 20: be_marg_hbm_kernel only; W = 20 has nobs > 16).  ring_base, the rotation of pre_idx and the seed vary with the case."""
    out = []
    for i, F0 in enumerate(F0_LIST):
        out.append(("F0_%d_W4" % F0, 4, dict(F0=F0, ring_base=1 + i % 4, rot_pre=1 + (i + 2) % 4, seed=i)))
    for i, F0 in enumerate([0, 17, 33, 65]):
        out.append(("F0_%d_W10" % F0, 10, dict(F0=F0, ring_base=3 + i, rot_pre=2 + i, seed=20 + i)))
    for i, (name, kw) in enumerate(sorted(KINDS.items())):
        for W in (4, 10):
            out.append(("%s_W%d" % (name, W), W, dict(kw, ring_base=1 + (i + 1) % W, rot_pre=1 + i % W, seed=40 + i)))
    out.append(("wide_W12", 12, dict(F0=33, ring_base=5, rot_pre=7, seed=70, estimate_td=1, tr=0.02)))
    out.append(("wide_W20", 20, dict(F0=17, ring_base=11, rot_pre=13, seed=71)))
    out.append(("wide_W20_moved", 20, dict(F0=5, ring_base=20, rot_pre=1, seed=72, moved=1)))
    return out


CASES = {name: (W, kw) for name, W, kw in case_list()}
# what each case is named for: the route of the m-block's pseudo-inverse and the landmarks under the cut
EIGEN_ROUTE = {n for n in CASES if n.startswith(("no_imu", "long_dt"))}
NOOP = {n for n in CASES if n.startswith(("second_new_noop", "second_new_no_prior"))}
N_FLAT = {n: CASES[n][1].get("flat", 0) for n in CASES}


def cfg_kwargs(name):
    """the configuration fields a case's handle needs beyond the window size"""
    W, kw = CASES[name]
    return dict(window_size=W, estimate_td=int(kw.get("estimate_td", 0)), use_imu=int(kw.get("use_imu", 1)), tr=float(kw.get("tr", 0.0)),
                max_landmarks=256)


# Cases left out of the c0 comparison, and why (tests/test_marg_default_ref_cpu.py::test_c0_list pins that these, and only these, are undetermined
# already for float64 numpy's H): a first marginalisation without a prior leaves the four gauge directions (position and yaw of the whole window) with
# eigenvalues of H at round-off, of either sign; delta = 64 eps n max|diag H| lifts them to within the Cholesky solve's own backward error of zero
# (rho >= 1/2 in c0_self, or no factor at all), so whether the factorisation succeeds -- the kernel returns 0 when it does not -- and what it returns
# are both decided by rounding.  Everything else of these cases (A, b, A_r, b_r, prior_H, prior_r, prior_x0, the mask) is compared.
C0_UNDETERMINED = ("long_dt_W10", "long_dt_W4", "no_imu_W10", "no_imu_W4", "no_prior_W10", "no_prior_W4")


def c0_self_ratio(name, H, rr, c0):
    """error / bound of a returned c0 against c0_self of the returned (H, r); asserts that the bound exists for every case outside C0_UNDETERMINED
    (None inside it)"""
    cs, bound, rho, pd = c0_self(H, rr)
    if name in C0_UNDETERMINED:
        return None
    assert pd and rho < 0.5, (name, rho, pd)
    e = abs(float(c0) - cs)
    return 0.0 if e == 0 else e / bound


_case_cache, _ref_cache = {}, {}


def get_case(name, cfg):
    if name not in _case_cache:
        W, kw = CASES[name]
        _case_cache[name] = make_case(cfg, W=W, **kw)
    return _case_cache[name]


def get_ref(name, cfg):
    if name not in _ref_cache:
        _ref_cache[name] = reference(get_case(name, cfg), cfg)
    return _ref_cache[name]
