"""High-precision references for the dense FP64 primitives of be_linalg.h (tests/test_gpu_linalg_prims.py).

Everything up to n = 32 is computed with mpmath at 40 significant digits from the float64 input as given, so the reference carries no
float64 round-off of its own.  Beyond that, where mpmath would be too slow, the eigen-decomposition falls back to LAPACK in float64
(`eigh_ref` says which it used); the tests only take that path for well-conditioned matrices and account for LAPACK's own backward error.
Residuals and orthogonality of a float64 result are formed in np.longdouble (64-bit mantissa on x86-64), so their own rounding is far
below the float64 tolerances they are checked against.
"""
import mpmath
import numpy as np

DPS = 40
MP_MAX = 32          # largest n handed to mpmath
EPS = np.finfo(np.float64).eps


def _mp(A):
    return mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in np.asarray(A, np.float64)])


def mp_eigh(A):
    """Eigenvalues (ascending) and orthonormal eigenvectors (columns) of the symmetric float64 matrix A at DPS digits, rounded to float64."""
    A = np.asarray(A, np.float64)
    with mpmath.workdps(DPS):
        E, Q = mpmath.eigsy(_mp(A))
        w = np.array([float(E[i]) for i in range(A.shape[0])])
        V = np.array([[float(Q[i, j]) for j in range(A.shape[0])] for i in range(A.shape[0])])
    o = np.argsort(w)
    return w[o], V[:, o]


def eigh_ref(A):
    """(eigenvalues ascending, eigenvectors, source): mpmath for n <= MP_MAX, LAPACK float64 (numpy.linalg.eigh) beyond."""
    A = np.asarray(A, np.float64)
    if A.shape[0] <= MP_MAX:
        w, V = mp_eigh(A)
        return w, V, "mpmath"
    w, V = np.linalg.eigh(A)      # LAPACK float64: only for large well-conditioned cases, error ~ n eps |A|_2 of its own
    return w, V, "lapack"


def mp_inv(A):
    A = np.asarray(A, np.float64)
    with mpmath.workdps(DPS):
        M = _mp(A) ** -1
        return np.array([[float(M[i, j]) for j in range(A.shape[0])] for i in range(A.shape[0])])


def mp_lambda_min(A):
    """Smallest eigenvalue of the symmetric float64 matrix A, as an mpf at DPS digits (exact comparisons with a float64 floor)."""
    with mpmath.workdps(DPS):
        E = mpmath.eigsy(_mp(A), eigvals_only=True)
        return min(E[i] for i in range(len(E)))


def mp_pinv_cut(A, cut):
    """Truncated pseudo-inverse of MarginalizationInfo::marginalize: V diag(1/lambda if lambda > cut else 0) V^T, at DPS digits."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    with mpmath.workdps(DPS):
        E, Q = mpmath.eigsy(_mp(A))
        D = mpmath.matrix(n, n)
        for k in range(n):
            D[k, k] = 1 / E[k] if E[k] > cut else 0
        M = Q * D * Q.T
        return np.array([[float(M[i, j]) for j in range(n)] for i in range(n)])


def mp_cholesky(A):
    """Lower Cholesky factor at DPS digits (n <= MP_MAX), None if a pivot is not positive."""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    with mpmath.workdps(DPS):
        M = _mp(A)
        L = mpmath.matrix(n, n)
        for j in range(n):
            d = M[j, j] - sum(L[j, k] ** 2 for k in range(j))
            if d <= 0:
                return None
            L[j, j] = mpmath.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (M[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
        return np.array([[float(L[i, j]) for j in range(n)] for i in range(n)])


def norm2(A):
    """Spectral norm of a symmetric matrix (largest |eigenvalue|), from the reference decomposition."""
    w, _, _ = eigh_ref(A)
    return float(np.abs(w).max()) if len(w) else 0.0


def residual(A, w, V):
    """max |A V - V diag(w)| formed in long double."""
    Al, Vl, wl = (np.asarray(x, np.longdouble) for x in (A, V, w))
    return float(np.abs(Al @ Vl - Vl * wl[None, :]).max())


def orthogonality(V):
    """max |V^T V - I| formed in long double."""
    Vl = np.asarray(V, np.longdouble)
    return float(np.abs(Vl.T @ Vl - np.eye(V.shape[1], dtype=np.longdouble)).max())


def exclusive_scan(flags):
    f = np.asarray(flags, np.int64)
    return (np.cumsum(f) - f).astype(np.int64), int(f.sum())


# ---- test matrices
def random_symmetric(n, seed):
    B = np.random.default_rng(seed).standard_normal((n, n))
    return B + B.T


def with_spectrum(lam, seed):
    """Q diag(lam) Q^T with a random orthogonal Q, symmetrised bit for bit."""
    n = len(lam)
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    A = (Q * np.asarray(lam, np.float64)) @ Q.T
    return 0.5 * (A + A.T)


def psd_null(n, rank, seed):
    """Positive semi-definite matrix with an exact null space of dimension n - rank: G = J^T J (rank x rank) with rows and columns duplicated,
    so rows k >= rank repeat row k mod rank bit for bit and e_k - e_(k mod rank) are exact null vectors."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((2 * rank, rank))
    G = J.T @ J
    G = 0.5 * (G + G.T)
    m = np.arange(n) % rank
    return np.ascontiguousarray(G[np.ix_(m, m)])


def schur_ref(H, Ws, inv, dgp, sp, mu):
    """(S, bound) of be_solve's Schur complement S = S_p H S_p + mu diag(dgp^2) - sum_k inv[k] (S_p W[k])^T (S_p W[k]) in long double, a column with
    sp = 0 an identity row; bound[r, c] = gamma_m sum |terms| with m = Kpad + 6 (the roundings of one product plus the summation of Kpad + 2
    terms): what any order of float64 evaluation stays within."""
    L = np.longdouble
    H, Ws, inv, dgp, sp = (np.asarray(x, L) for x in (H, Ws, inv, dgp, sp))
    n, K = H.shape[0], Ws.shape[0]
    S0 = sp[:, None] * sp[None, :] * H
    D = mu * dgp * dgp
    S0[np.diag_indices(n)] += D
    A0 = np.abs(sp[:, None] * sp[None, :] * H)
    A0[np.diag_indices(n)] += np.abs(D)
    SW = Ws * sp[None, :]
    S = S0 - (SW * inv[:, None]).T @ SW
    A = A0 + (np.abs(SW) * np.abs(inv)[:, None]).T @ np.abs(SW)
    z = np.where(sp == 0)[0]
    S[z, z] = 1.0
    A[z, z] = 0.0
    m = K + 6
    gamma = m * EPS / (1 - m * EPS)
    return S, gamma * A
