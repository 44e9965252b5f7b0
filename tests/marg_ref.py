"""The literal marginalisation (vio_config.marg_exact = 1 / 2; be_kernels.hip marg_exact_finish, marg_literal_prior, marg_certificate) by its
definition, in plain high-precision numpy / mpmath, with the inputs and the error bounds of tests/test_gpu_marg_literal.py.
tests/test_marg_ref_cpu.py checks this module against itself without a GPU.

The definition (MarginalizationInfo::marginalize).  q = [md | n] are the pose / speed-bias of frame 0 and the kept parameters, the F0 landmarks that
start in frame 0 follow; m = md + F0 is the marginalised block.
    A_mm  = [[sym(A[:md, :md]), B^T], [B, diag(d)]],  B = Cl[:, :md]          (only the md x md block is symmetrised, as the device code does)
    X     = A_mm^+ = V diag(1 / lambda if lambda > 1e-8 else 0) V^T
    A_rm  = [A[md:, :md] | Cl[:, md:]^T],  A_mr = [A[:md, md:]; Cl[:, md:]],  b_m = [b[:md]; gl]
    A_r   = A[md:, md:] - (A_rm X) A_mr,   b_r = b[md:] - (A_rm X) b_m
    sym(A_r) = V2 diag(lambda2) V2^T, K = {k: lambda2_k > 1e-8};  J = rows sqrt(lambda2_k) v_k^T (zero rows for k not in K),
    rf_k = (v_k . b_r) / sqrt(lambda2_k) (0 for k not in K);  prior_H = J^T J, prior_r = J^T rf = P_K b_r, prior_c0 = |rf|^2 = b_r^T sym(A_r)_K^+ b_r.

References.
  * m <= 32 (linalg_ref.MP_MAX): mpmath at 40 digits on the float64 input as given: eigsy of A_mm, the cut, the products.
  * larger m: only inputs whose A_mm has no eigenvalue near the cut apart from EXACT zeros (landmarks with d = 0 and a zero coupling row: unit
    eigenvectors, the reference deletes them).  A_mm^+ is then the inverse of the rest, formed by block elimination -- landmarks 1 / d, the md x md
    Schur complement by Gaussian elimination with partial pivoting -- in np.longdouble (`block_inverse`).  lambda_kept_min = 1 / |X|_2 is taken
    from that inverse and asserted >= 1e-4; where |A_mm|_2 <= 1e3 numpy.linalg.eigvalsh must agree (its own error m eps |A_mm| is far below 1e-4).
    `block_inverse` is written for any scalar type: at m <= 32 the CPU test runs it on mpmath numbers and finds the eigsy route again to 1e-25
    relative (the route is the definition), and in np.longdouble to that format's precision (C m 2^-63 cond(A_mm)).
  * second half for n > 32: A_r = fl(Q diag(lambda) Q^T) with Q orthonormal to long-double precision and lambda prescribed, both formed in long double,
    so the kept part is Q_K diag(lambda_K) Q_K^T without an eigen-solver.  Rounding A_r to float64 moves it by e_ref <= eps / 2 |A_r|_F, the
    reference's own error, which enters the bounds below beside the solver's backward error.  n <= 32: mpmath on the float64 A_r, e_ref = 0.
  * psd_null (exact null space by duplicated rows, linalg_ref.psd_null): the kept part of A_r is A_r itself and P_K the projector on the range of
    the duplication matrix, both exact; c0 through a long-double inverse of the rank x rank generator.

Bounds.  C = 8 (CTOL of tests/test_gpu_linalg_prims.py), eps = 2^-52, gamma_k = k eps / (1 - k eps); |.|_2 is the spectral norm, and matrix errors are
measured in it (it bounds every entry).  A backward-stable symmetric eigen-solver returns the exact decomposition of M + E, |E|_2 <= C k eps |M|_2.
  X = A_mm^+        |dX|_2 <= bx = C m eps |A_mm|_2 / lambda_kept_min^2          (Wedin: (1 + sqrt 5) / 2 |X|_2^2 |E|_2 for equal rank; the cut keeps
                    the rank since the dropped eigenvalues are at round-off, far below 1e-8, and the kept ones >= 1e-4 or prescribed)
  A_r[i, j]         bx |A_rm[i, :]|_2 |A_mr[:, j]|_2  +  gamma_(m+1) (|A_rr[i, j]| + 2 (|A_rm| |X| |A_mr|)[i, j])
                    (first order in dX through the two products; each of the two products is a sum of at most m + 1 terms, and
                    |fl(A_rm X)| <= (1 + gamma_m) |A_rm| |X| puts both under the one sum of absolute terms)
  b_r[i]            bx |A_rm[i, :]|_2 |b_m|_2  +  gamma_(m+1) (|b[md + i]| + 2 (|A_rm| |X| |b_m|)[i])
  prior_H           |dH|_2 <= E k_gap,  E = C n eps |A_r|_2 + e_ref,  k_gap = lambda_kept_min / (lambda_kept_min - lambda_drop_max)
                    (H~ - H = E P~ + A (P~ - P); to first order A (P~ - P) couples kept k and dropped d with weight lambda_k / (lambda_k - lambda_d),
                    largest at lambda_kept_min; k_gap >= 1 covers the first term within C)
  prior_r = P b_r   |dr|_2 <= E |b_r|_2 / gap,  gap = lambda_kept_min - lambda_drop_max      (Davis-Kahan: |P~ - P|_2 <= |E|_2 / gap)
  prior_c0          |dc0| <= E |b_r|_2^2 / lambda_kept_min^2                                 (as for X)
  prior_J, prior_rf checked through J^T J, J^T rf, |rf|^2 against the RETURNED prior_H, prior_r, prior_c0, entrywise within gamma_n of the sums of
                    absolute terms (formed in long double); the rows themselves have free signs and order.  The number of non-zero rows of J equals
                    the number of kept eigenvalues.
  certificate       bound = |Pinv|_F + 2 sqrt(n_t) + sqrt(n_d) + sqrt(n_db) sqrt(n_t) (be_kernels.hip marg_certificate) agrees with its long-double
                    value to C (F0 + md) eps relative: sums of squares of up to F0 md products.  The inner sum tt = sum_b Pinv[a, b] Cl[l, b] is the
                    one signed sum; its error gamma_md dinv |Pinv[a, :]|_2 |Cl[l, :]|_2 moves the bound by at most
                    (2 + x) x md eps |Pinv|_F with x = sqrt(n_db), inside the figure whenever (2 + x) x md <= C (F0 + md) / 2: `cert_case`
                    asserts that of every input.

Worst error / bound of a float64 numpy evaluation of the literal algorithm (numpy.linalg.eigh; `np_part0`, `np_part1`, `np_cert`) on every input of the
GPU test: see the docstring of tests/test_marg_ref_cpu.py.
"""
import functools

import mpmath
import numpy as np

import linalg_ref as R

L = np.longdouble
EPS = R.EPS
C = 8
CUT = 1e-8
TWO_M26 = 2.0 ** -26          # 1.49e-8: the kept partner of 1e-8 in the strictness cases


def gamma(k):
    return k * EPS / (1 - k * EPS)


def norm2(M):
    M = np.asarray(M, np.float64)
    return float(np.linalg.norm(M, 2)) if M.size else 0.0


# ------------------------------------------------------------------------------------------------------------ scalar-type generic algebra
def _zeros(shape, like):
    if like.dtype == object:
        Z = np.empty(shape, object)
        Z[...] = mpmath.mpf(0)
        return Z
    return np.zeros(shape, like.dtype)


def gauss_inverse(S):
    """Inverse by Gauss-Jordan elimination with partial pivoting, in the scalar type of S (np.longdouble, or object = mpmath numbers)."""
    k = S.shape[0]
    M = _zeros((k, 2 * k), S)
    M[:, :k] = S
    for i in range(k):
        M[i, k + i] = M[i, k + i] + 1
    for c in range(k):
        p = c + int(np.argmax([abs(M[r, c]) for r in range(c, k)]))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(k):
            if r != c:
                M[r] = M[r] - M[c] * M[r, c]
    return M[:, k:].copy()


def block_inverse(Pm, B, d):
    """[[Pm, B^T], [B, diag(d)]]^-1 by block elimination in the scalar type of the arguments: landmarks 1 / d, then the Schur complement of the
    md x md block by Gaussian elimination.  Every d must be non-zero."""
    md, F0 = Pm.shape[0], len(d)
    if F0 == 0:
        return gauss_inverse(Pm)
    di = 1 / d
    DB = B * di[:, None]                     # D^-1 B  (F0 x md)
    Si = gauss_inverse(Pm - B.T @ DB)        # S^-1
    T = Si @ DB.T                            # S^-1 B^T D^-1  (md x F0)
    X = _zeros((md + F0, md + F0), Pm)
    X[:md, :md] = Si
    X[:md, md:] = -T
    X[md:, :md] = -T.T
    X[md:, md:] = DB @ T
    for l in range(F0):
        X[md + l, md + l] = X[md + l, md + l] + di[l]
    return X


def to_mp(A):
    A = np.asarray(A, np.float64)
    out = np.empty(A.shape, object)
    for idx in np.ndindex(A.shape):
        out[idx] = mpmath.mpf(float(A[idx]))
    return out


def mp_to_ld(M):
    """mpmath numbers to np.longdouble through a float64 head and tail (106 bits, more than the format holds)."""
    out = np.zeros(M.shape, L)
    for idx in np.ndindex(M.shape):
        hi = float(M[idx])
        out[idx] = L(hi) + L(float(M[idx] - mpmath.mpf(hi)))
    return out


# ------------------------------------------------------------------------------------------------------------ part 0: inputs
class System:
    """A marginalisation-shaped system: A (mq x mq), b (mq), Cl (F0 x ldc, columns >= mq NaN), d, gl (F0)."""

    def __init__(self, md, n, A, b, Cl, d, gl, ldc):
        self.md, self.n, self.F0, self.ldc = md, n, len(d), ldc
        self.m, self.mq = md + len(d), md + n
        self.A, self.b, self.d, self.gl = (np.ascontiguousarray(x, np.float64) for x in (A, b, d, gl))
        self.Cl = np.full((max(self.F0, 1), ldc), np.nan)
        self.Cl[:self.F0, :self.mq] = Cl
        self.Cl = self.Cl[:self.F0] if self.F0 else np.zeros((0, ldc))

    def parts(self):
        """(Pm, B, d, A_rm, A_mr, A_rr, b_m, b_r0) in float64, literally as the device code reads them."""
        md, mq = self.md, self.mq
        Pm = 0.5 * (self.A[:md, :md] + self.A[:md, :md].T)
        Cq = self.Cl[:, :mq]
        B = Cq[:, :md]
        Arm = np.hstack([self.A[md:, :md], Cq[:, md:].T])
        Amr = np.vstack([self.A[:md, md:], Cq[:, md:]])
        return Pm, B, self.d, Arm, Amr, self.A[md:, md:], np.concatenate([self.b[:md], self.gl]), self.b[md:]

    def Amm(self):
        Pm, B, d = self.parts()[:3]
        return np.block([[Pm, B.T], [B, np.diag(d)]]) if self.F0 else Pm.copy()


def system(md, F0, n, seed, kind="well", ldc=None, drop=0, cut_pair=None):
    """J^T J of a random tall J in which a row meets at most one landmark, so the landmark block is diagonal and the whole matrix is PSD.
    kind: well (cond(A_mm) <= 1e3) | graded (d over 1e-2 .. 1e10) | null (pose columns 0 and 1 duplicated: an exact null direction) |
    asym (A not symmetric) | diag (A_mm diagonal).  drop: the LAST `drop` landmarks have d = 0 and a zero row.  cut_pair = (lo, hi): the last two
    landmarks get d = lo, hi and zero rows."""
    rng = np.random.default_rng([seed, md, F0, n])
    mq = md + n
    ldc = mq + 5 if ldc is None else ldc
    nz = (2 if cut_pair else 0) + drop          # landmarks with a zero row
    Fa = F0 - nz
    assert Fa >= 0
    k = 4 * mq
    G = rng.standard_normal((k, mq)) / np.sqrt(k)
    if kind == "diag":
        G = np.zeros((mq, mq))
        G[np.arange(mq), np.arange(mq)] = np.sqrt(np.linspace(0.5, 2.0, mq))
        G[md:, md:] += 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)      # (the kept block stays full)
        k = mq
    s = 0.7 / np.sqrt(3 * max(Fa, 1))
    U = s * rng.standard_normal((Fa, 3, mq)) * (0.0 if kind == "diag" else 1.0)
    w = 1.0 + 0.2 * rng.standard_normal((Fa, 3))
    if kind == "graded":
        w *= np.sqrt(np.logspace(-2, 10, Fa))[rng.permutation(Fa)][:, None] if Fa else 1.0
    res = rng.standard_normal(k + 3 * Fa)
    Jq = np.vstack([G, U.reshape(3 * Fa, mq)])
    M = Jq.T @ Jq
    M = 0.5 * (M + M.T)
    Cl = np.einsum("lr,lrq->lq", w, U)
    d = np.einsum("lr,lr->l", w, w)
    b = Jq.T @ res
    gl = np.einsum("lr,lr->l", w, res[k:].reshape(Fa, 3))
    if kind == "null":
        idx = np.arange(mq)
        idx[1] = 0
        M, b, Cl = M[np.ix_(idx, idx)], b[idx], Cl[:, idx]
    if kind == "asym":
        M = M + 1e-3 * rng.standard_normal((mq, mq))
    tail = ([cut_pair[0], cut_pair[1]] if cut_pair else []) + [0.0] * drop
    Cl = np.vstack([Cl, np.zeros((nz, mq))])
    d = np.concatenate([d, tail])
    gl = np.concatenate([gl, np.zeros(nz)])
    return System(md, n, M, b, Cl, d, gl, ldc)


def with_zero_landmarks(sys0, F0):
    """sys0 (F0 = 0) with F0 landmarks of d = 0 and zero rows appended: the same A and b, so the same pose block of A_mm^+."""
    assert sys0.F0 == 0
    return System(sys0.md, sys0.n, sys0.A, sys0.b, np.zeros((F0, sys0.mq)), np.zeros(F0), np.zeros(F0), sys0.ldc)


# ------------------------------------------------------------------------------------------------------------ part 0: reference
class Ref0:
    pass


def pinv_mp(Amm):
    """The literal truncated pseudo-inverse at 40 digits: (X as mpmath numbers, kept eigenvalues, dropped eigenvalues)."""
    m = Amm.shape[0]
    with mpmath.workdps(R.DPS):
        E, Q = mpmath.eigsy(mpmath.matrix(to_mp(Amm).tolist()))
        D = mpmath.matrix(m, m)
        for k in range(m):
            D[k, k] = 1 / E[k] if E[k] > CUT else 0
        X = Q * D * Q.T
        Xo = np.empty((m, m), object)
        for i in range(m):
            for j in range(m):
                Xo[i, j] = X[i, j]
        ev = [E[k] for k in range(m)]
    return Xo, [float(e) for e in ev if e > CUT], [float(e) for e in ev if not e > CUT]


def pinv_ld(sys):
    """Long-double route: exact-zero landmarks (d <= CUT with an all-zero row) deleted, the rest inverted by block elimination.
    (X, kept mask over m).  Asserts that what it deletes is exactly decoupled."""
    Pm, B, d = sys.parts()[:3]
    gone = d <= CUT
    assert not np.any(sys.Cl[gone, :sys.mq]), "a dropped landmark must have a zero row"
    keep = np.concatenate([np.ones(sys.md, bool), ~gone])
    Xk = block_inverse(Pm.astype(L), B[~gone].astype(L), d[~gone].astype(L))
    X = np.zeros((sys.m, sys.m), L)
    X[np.ix_(keep, keep)] = Xk
    return X, keep


def ref_part0(sys, route=None):
    """Reference of part 0: X, A_r, b_r in long double with their bounds.  route: "mp" | "ld" | None (mp for m <= 32)."""
    route = route or ("mp" if sys.m <= R.MP_MAX else "ld")
    Pm, B, d, Arm, Amr, Arr, bm, br0 = sys.parts()
    Amm = sys.Amm()
    r = Ref0()
    r.route, r.m, r.n = route, sys.m, sys.n
    if route == "mp":
        with mpmath.workdps(R.DPS):
            Xo, kept, dropped = pinv_mp(Amm)
            X = mp_to_ld(Xo)
        r.X_mp = Xo
        r.lam_kept_min = min(kept)
        r.lam_drop_max = max(dropped) if dropped else None
        r.n_dropped = len(dropped)
    else:
        X, keep = pinv_ld(sys)
        r.lam_kept_min = 1.0 / norm2(X.astype(np.float64))
        r.n_dropped = int((~keep).sum())
        r.lam_drop_max = 0.0 if r.n_dropped else None
        assert r.lam_kept_min >= 1e-4, ("the long-double route needs A_mm far from the cut", r.lam_kept_min)
    r.normA = norm2(Amm)
    if route == "ld" and r.normA <= 1e3:
        w = np.linalg.eigvalsh(Amm)
        assert w[r.n_dropped] >= 1e-4 and abs(w[r.n_dropped] - r.lam_kept_min) <= 1e-6 * r.lam_kept_min + sys.m * EPS * r.normA, (w[:r.n_dropped + 1], r.lam_kept_min)
    r.X = X
    m, n = sys.m, sys.n
    r.bx = C * m * EPS * r.normA / r.lam_kept_min ** 2
    ArmL, AmrL, bmL = Arm.astype(L), Amr.astype(L), bm.astype(L)
    T1 = ArmL @ X
    r.Ar = Arr.astype(L) - T1 @ AmrL
    r.br = br0.astype(L) - T1 @ bmL
    absT = np.abs(ArmL) @ np.abs(X)
    rn = np.sqrt((ArmL * ArmL).sum(axis=1)).astype(np.float64)
    cn = np.sqrt((AmrL * AmrL).sum(axis=0)).astype(np.float64)
    g = gamma(m + 1)
    r.Ar_bound = r.bx * rn[:, None] * cn[None, :] + g * (np.abs(Arr) + 2 * (absT @ np.abs(AmrL)).astype(np.float64))
    r.br_bound = r.bx * rn * float(np.sqrt((bmL * bmL).sum())) + g * (np.abs(br0) + 2 * (absT @ np.abs(bmL)).astype(np.float64))
    return r


def np_part0(sys):
    """The literal algorithm in float64 numpy (numpy.linalg.eigh): X, A_r, b_r."""
    Pm, B, d, Arm, Amr, Arr, bm, br0 = sys.parts()
    w, V = np.linalg.eigh(sys.Amm())
    X = (V * np.where(w > CUT, 1.0 / np.where(w > CUT, w, 1.0), 0.0)) @ V.T
    T1 = Arm @ X
    return X, Arr - T1 @ Amr, br0 - T1 @ bm


def check_part0(ref, X, Ar, br):
    """Worst error / bound of (X, A_r, b_r) against the reference: dict of ratios."""
    out = {}
    D = X.astype(L) - ref.X
    if hasattr(ref, "i_hi"):      # the landmark just above the cut: 1 / lambda of an eigenvalue the solver knows to C m eps |A_mm|_2
        out["hi"] = abs(X[ref.i_hi, ref.i_hi] * ref.d_hi - 1.0) / (C * ref.m * EPS * ref.normA / ref.d_hi)
        D[ref.i_hi, ref.i_hi] = 0
    return {**out, "X": norm2(D.astype(np.float64)) / ref.bx,
            "A_r": float(np.max(np.abs(Ar.astype(L) - ref.Ar).astype(np.float64) / ref.Ar_bound)),
            "b_r": float(np.max(np.abs(br.astype(L) - ref.br).astype(np.float64) / ref.br_bound))}


# ------------------------------------------------------------------------------------------------------------ part 1: inputs and reference
class Ref1:
    pass


def _orthonormal_ld(n, seed):
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    Q = Q.astype(L)
    for _ in range(2):                                   # Newton-Schulz: orthogonality error e -> 3/8 e^2, down to the format's round-off
        Q = Q @ (1.5 * np.eye(n, dtype=L) - 0.5 * (Q.T @ Q))
    return Q


def spectrum(kind, n):
    """Prescribed eigenvalues of A_r.  kept: all far above the cut; gauge: kept >= 1e-6 with min(6, n // 3) dropped ones <= 1e-10 (the gauge
    directions of the real prior); neg: as gauge with the dropped ones at -1e-12."""
    nd = 0 if kind == "kept" else min(6, n // 3)
    if kind == "kept":
        return np.logspace(-3, 2, n) if n > 1 else np.array([3.0])
    hi = np.logspace(-6, 2, n - nd) if n - nd > 1 else np.array([2.0])
    lo = np.resize([1e-10, 1e-12, 0.0, 1e-14, 1e-11, 1e-16], nd) if kind == "gauge" else np.full(nd, -1e-12)
    return np.concatenate([lo, hi])


def _finish_ref1(r, A, b, H, Pb, c0, kept, dropped, e_ref):
    n = A.shape[0]
    r.A, r.b, r.n = A, b, n
    r.H, r.Pb, r.c0 = H, Pb, c0
    r.n_kept = len(kept)
    r.lam_kept_min = float(min(kept)) if len(kept) else None
    r.lam_drop_max = float(max(dropped)) if len(dropped) else None
    r.normA = norm2(0.5 * (A + A.T))
    r.E = C * n * EPS * r.normA + e_ref
    if r.n_kept:
        gap = r.lam_kept_min - (r.lam_drop_max if len(dropped) else 0.0)
        nb = float(np.linalg.norm(b))
        r.H_bound = r.E * r.lam_kept_min / gap
        r.r_bound = r.E * nb / gap
        r.c0_bound = r.E * nb * nb / r.lam_kept_min ** 2
    return r


def ref1_mp(A, b):
    """Reference of the second half on the float64 (A, b) as given, at 40 digits (n <= 32)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    n = A.shape[0]
    with mpmath.workdps(R.DPS):
        As = to_mp(A)
        As = (As + As.T) / 2
        E, Q = mpmath.eigsy(mpmath.matrix(As.tolist()))
        bm = [mpmath.mpf(float(x)) for x in b]
        H = np.empty((n, n), object)
        H[...] = mpmath.mpf(0)
        Pb = np.empty(n, object)
        Pb[...] = mpmath.mpf(0)
        c0 = mpmath.mpf(0)
        kept, dropped = [], []
        for k in range(n):
            if E[k] > CUT:
                kept.append(float(E[k]))
                v = np.array([Q[i, k] for i in range(n)], object)
                vb = sum(v[i] * bm[i] for i in range(n))
                H = H + np.outer(v, v) * E[k]
                Pb = Pb + v * vb
                c0 += vb * vb / E[k]
            else:
                dropped.append(float(E[k]))
        H, Pb, c0 = mp_to_ld(H), mp_to_ld(Pb), mp_to_ld(np.array([c0], object))[0]
    r = Ref1()
    r.route = "mp"
    return _finish_ref1(r, A, b, H, Pb, c0, kept, dropped, 0.0)


def reduced(kind, n, seed=0):
    """(A_r, b_r) float64 and the by-construction long-double reference.  kind: kept | gauge | neg | null."""
    rng = np.random.default_rng([seed, n, sum(map(ord, kind))])
    b = rng.standard_normal(n)
    r = Ref1()
    r.route = "construction"
    if kind == "null":
        rank = max(1, (2 * n) // 3)
        A = R.psd_null(n, rank, 3000 + n + seed)
        G = A[:rank, :rank]
        idx = np.arange(n) % rank
        D = np.zeros((n, rank), L)
        D[np.arange(n), idx] = 1
        cnt = D.sum(axis=0)
        Gi = gauss_inverse(G.astype(L))
        y = (D.T @ b.astype(L)) / cnt                       # (D^T D)^-1 D^T b
        Pb = D @ y
        c0 = y @ (Gi @ y)
        sq = np.sqrt(cnt.astype(np.float64))
        kept = np.linalg.eigvalsh(sq[:, None] * G * sq[None, :])        # non-zero spectrum of D G D^T (well-conditioned: float64 serves the bound)
        return A, b, _finish_ref1(r, A, b, A.astype(L), Pb, c0, list(kept), [0.0] * (n - rank), 0.0)
    lam = spectrum(kind, n)
    Q = _orthonormal_ld(n, [seed, n, 7])
    Al = (Q * lam.astype(L)[None, :]) @ Q.T
    Al = 0.5 * (Al + Al.T)
    A = Al.astype(np.float64)
    keep = lam > CUT
    Qk, lk = Q[:, keep], lam[keep].astype(L)
    vb = Qk.T @ b.astype(L)
    H = (Qk * lk[None, :]) @ Qk.T
    e_ref = 0.5 * EPS * float(np.linalg.norm(A, "fro"))
    return A, b, _finish_ref1(r, A, b, H, Qk @ vb, (vb * vb / lk).sum(), list(lam[keep]), list(lam[~keep]), e_ref)


def ref1_all_kept(A, b):
    """Reference of the second half for an (A, b) whose sym(A) is positive definite far above the cut (lambda_min >= 1e-4 by numpy.linalg.eigvalsh,
    |A|_2 <= 1e3, so its own error n eps |A|_2 is far below): nothing is dropped, prior_H = sym(A), prior_r = b, c0 = b^T sym(A)^-1 b in long double.
    What part 0 hands its own second half is checked with it, on the A_r and b_r the device returned."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    As = 0.5 * (A.astype(L) + A.astype(L).T)
    w = np.linalg.eigvalsh(As.astype(np.float64))
    assert w[0] >= 1e-4 and w[-1] <= 1e3, (w[0], w[-1])
    bl = b.astype(L)
    r = Ref1()
    r.route = "all kept"
    return _finish_ref1(r, A, b, As, bl, bl @ (gauss_inverse(As) @ bl), list(w), [], 0.0)


def np_part1(A, b):
    """The literal second half in float64 numpy: J, rf, H, r, c0."""
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    S = np.where(w > CUT, w, 0.0)
    Si = np.where(w > CUT, 1.0 / np.where(w > CUT, w, 1.0), 0.0)
    J = np.sqrt(S)[:, None] * V.T
    rf = np.sqrt(Si) * (V.T @ b)
    return J, rf, J.T @ J, J.T @ rf, float(rf @ rf)


def check_part1(ref, J, rf, H, r, c0):
    """Worst error / bound of the second half's outputs: dict of ratios; `rows` = number of non-zero rows of J."""
    n = ref.n
    Jl, rl = J.astype(L), rf.astype(L)
    g = gamma(n)
    tiny = np.finfo(np.float64).tiny
    out = {"rows": int(np.any(J != 0, axis=1).sum())}
    out["JtJ"] = float(np.max(np.abs(Jl.T @ Jl - H.astype(L)).astype(np.float64) / (g * (np.abs(Jl).T @ np.abs(Jl)).astype(np.float64) + tiny)))
    out["Jtr"] = float(np.max(np.abs(Jl.T @ rl - r.astype(L)).astype(np.float64) / (g * (np.abs(Jl).T @ np.abs(rl)).astype(np.float64) + tiny)))
    out["rr"] = float(abs((rl * rl).sum() - L(c0)) / (g * float((rl * rl).sum()) + tiny))
    if ref.n_kept:
        out["H"] = norm2((H.astype(L) - ref.H).astype(np.float64)) / ref.H_bound
        out["r"] = float(np.linalg.norm((r.astype(L) - ref.Pb).astype(np.float64))) / ref.r_bound
        out["c0"] = float(abs(L(c0) - ref.c0)) / ref.c0_bound
    return out


PART1_KINDS = ["kept", "null", "gauge", "neg"]


def part1_sizes(M=114):
    return sorted({1, 2, 22, 76, M, M + 1, 128, 129, 136})


@functools.lru_cache(maxsize=None)
def part1_case(kind, n):
    """(A_r, b_r, reference): mpmath on the float64 input for n <= 32, by construction beyond."""
    A, b, r = reduced(kind, n)
    return (A, b, ref1_mp(A, b)) if n <= R.MP_MAX else (A, b, r)


def strict_diagonal(n, lo=CUT, hi=TWO_M26):
    """diag(lo, hi, 1, 1.5, ...) and b = 1, 2, ...: with lo = 1e-8 (not > 1e-8) row 0 of J and rf[0] are exactly zero, hi is kept."""
    dg = np.concatenate([[lo, hi], 1.0 + 0.5 * np.arange(n - 2)])[:n]
    return np.diag(dg), 1.0 + np.arange(n, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ part 2: the certificate
class Cert:
    pass


def cert_bound_ld(Pinv, Cl, dinv, second_new=False):
    """The bound expression of marg_certificate in long double."""
    P = Pinv.astype(L)
    n_s = (P * P).sum()
    n_t = n_d = n_db = L(0)
    if not second_new and len(dinv):
        md = P.shape[0]
        Bq, di = Cl[:, :md].astype(L), dinv.astype(L)
        T = (Bq @ P.T) * di[:, None]
        DB = Bq * di[:, None]
        n_t, n_d, n_db = (T * T).sum(), (di * di).sum(), (DB * DB).sum()
    return np.sqrt(n_s) + 2 * np.sqrt(n_t) + np.sqrt(n_d) + np.sqrt(n_db) * np.sqrt(n_t)


def np_cert(Pinv, Cl, dinv, pinv_direct=1, second_new=False):
    """marg_certificate in float64 numpy: (certified, bound)."""
    md = Pinv.shape[0]
    n_s = float((Pinv * Pinv).sum())
    n_t = n_d = n_db = 0.0
    bad = not pinv_direct
    if not second_new and len(dinv):
        bad = bad or not np.all(dinv > 0.0)
        T = (Cl[:, :md] @ Pinv.T) * dinv[:, None]
        DB = Cl[:, :md] * dinv[:, None]
        n_t, n_d, n_db = float((T * T).sum()), float((dinv * dinv).sum()), float((DB * DB).sum())
    bound = np.sqrt(n_s) + 2 * np.sqrt(n_t) + np.sqrt(n_d) + np.sqrt(n_db) * np.sqrt(n_t)
    return bool(not bad and np.isfinite(bound) and bound > 0.0 and 1.0 / bound > 1e-7), float(bound)


@functools.lru_cache(maxsize=None)
def cert_case(md, F0, lam_min, seed=0, ldc=None):
    """Inputs of the certificate for an A_mm = [[P, B^T], [B, D]] whose smallest eigenvalue is lam_min: a well-conditioned block of `system`
    shifted by a multiple of the identity.  Pinv = S^-1 (long double, rounded), dinv = 1 / d; columns >= md of Cl are NaN (never read)."""
    s = system(md, F0, 4, 900 + seed, "well")
    Pm, B, d = s.parts()[:3]
    lam0 = float(np.linalg.eigvalsh(s.Amm())[0])
    sh = lam_min - lam0
    Pm = Pm + sh * np.eye(md)
    d = d + sh
    c = Cert()
    c.md, c.F0, c.ldc = md, F0, (md + 3 if ldc is None else ldc)
    c.Amm = np.block([[Pm, B.T], [B, np.diag(d)]]) if F0 else Pm
    X = block_inverse(Pm.astype(L), B.astype(L), d.astype(L))
    c.Pinv = np.ascontiguousarray(X[:md, :md].astype(np.float64))
    c.Pinv = 0.5 * (c.Pinv + c.Pinv.T)
    c.dinv = (1 / d.astype(L)).astype(np.float64)
    c.Cl = np.full((F0, c.ldc), np.nan)
    c.Cl[:, :md] = B
    c.lam_min = float(R.mp_lambda_min(c.Amm)) if md + F0 <= R.MP_MAX else 1.0 / norm2(X.astype(np.float64))
    c.bound = cert_bound_ld(c.Pinv, c.Cl, c.dinv)
    c.inv_bound = float(1 / c.bound)
    x = float(np.sqrt(((B * c.dinv[:, None]) ** 2).sum())) if F0 else 0.0
    assert (2 + x) * x * md <= C * (F0 + md) / 2, ("the certificate's relative bound needs a moderate |D^-1 B|_F", x)
    return c


CERT_SIZES = [(15, 0), (15, 1), (15, 17), (6, 3), (15, 200), (15, 480)]
CERT_SWEEP = [1e-9, 1e-8, 4e-8, 5e-7, 1e-6, 1e-5, 1e-4, 1e-3]


# ------------------------------------------------------------------------------------------------------------ the cases of the GPU test
MXL_EXPECTED = 114      # what a handle chooses on the MI355X (160 KB of LDS, be_marg_exact_kernel's static 46480 bytes); the GPU test uses the value the
#                         harness returns, the CPU test covers this one

P0_N = 22


def part0_sizes(M=MXL_EXPECTED):
    """(md, F0, n, forced mxl) of part 0."""
    out = [(6, 0, P0_N, 0)] + [(15, F0, P0_N, 0) for F0 in (0, 1, 2, 16, 17)]
    out += [(15, 40 - 15, P0_N, 40), (15, 41 - 15, P0_N, 40)]
    out += [(15, m - 15, P0_N, 0) for m in sorted({M, M + 1, 128, 129, 215})]
    return out


def part0_kinds(md, F0):
    """The kinds of input that exist at a size: an exact null direction only where mpmath is the reference, landmark kinds where there are landmarks."""
    kinds = ["well", "asym"] + (["null"] if md + F0 <= R.MP_MAX else [])
    kinds += ["graded", "drop1", "dropall"] if F0 >= 1 else []
    kinds += ["strict", "strict_general"] if F0 >= 2 else []
    return kinds + (["drop3"] if F0 >= 3 else [])


@functools.lru_cache(maxsize=None)
def part0_case(kind, md, F0, n):
    """One input of part 0 with its reference: kind = well | graded | drop1 | drop3 | dropall | null | asym | strict | strict_general."""
    if kind in ("well", "graded", "null", "asym"):
        s = system(md, F0, n, 11, kind)
    elif kind in ("drop1", "drop3"):
        s = system(md, F0, n, 12, "well", drop=int(kind[4:]))
    elif kind == "dropall":
        s = with_zero_landmarks(system(md, 0, n, 11, "well"), F0)
    elif kind == "strict":            # A_mm diagonal: the solvers return its diagonal exactly, 1e-8 is dropped and 2^-26 kept
        s = system(md, F0, n, 13, "diag", cut_pair=(CUT, TWO_M26))
    elif kind == "strict_general":    # full pose block: the shifts of QL cost the last bits of a small eigenvalue, so the pair straddles the cut by 10 %
        s = system(md, F0, n, 13, "well", cut_pair=(0.9e-8, 1.1e-8))
    else:
        raise ValueError(kind)
    return s


@functools.lru_cache(maxsize=None)
def part0_ref(kind, md, F0, n):
    s = part0_case(kind, md, F0, n)
    if kind in ("strict", "strict_general"):
        return ref_strict(s)
    return ref_part0(s)


def ref_strict(s):
    """Reference where the last two landmarks have zero rows and d = (lo, hi) beside the cut: they are decoupled from the rest exactly, so X, A_r
    and b_r are those of the system without them (with its bounds, at the full m), X[lo, lo] = 0 and X[hi, hi] = 1 / hi.  r.i_lo, r.i_hi: their
    rows in X; the test compares those two entries on their own."""
    lo, hi = s.d[-2], s.d[-1]
    assert lo <= CUT < hi and not np.any(s.Cl[-2:, :s.mq])
    sub = System(s.md, s.n, s.A, s.b, s.Cl[:-2, :s.mq], s.d[:-2], s.gl[:-2], s.ldc)
    r = ref_part0(sub)
    X = np.zeros((s.m, s.m), L)
    X[:sub.m, :sub.m] = r.X
    X[s.m - 1, s.m - 1] = 1 / L(hi)
    scale = s.m / sub.m * gamma(s.m + 1) / gamma(sub.m + 1)
    r.X, r.m, r.i_lo, r.i_hi, r.d_hi = X, s.m, s.m - 2, s.m - 1, float(hi)
    r.n_dropped += 1
    r.bx, r.Ar_bound, r.br_bound = r.bx * scale, r.Ar_bound * scale, r.br_bound * scale
    return r
