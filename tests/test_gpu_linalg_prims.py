"""The dense FP64 primitives of be_linalg.h on their own, through the stage harnesses of stage_linalg.hip (each calls the routine directly), against the
high-precision references of tests/linalg_ref.py: the Jacobi solvers (jacobi_small, jacobi_block, jacobi_wave16), the LDS / HBM Householder + QL pair
(sym_eig_tridiag / sym_eig_tridiag_mt + tridiag_ql_wave), the certified inverse of be_marg's fast path (spd_inverse_wave16), the HBM blocked Cholesky
of be_solve (chol_blocked / chol_solve_blocked) and block_scan_flags.

Tolerances come from the bounds of backward-stable eigen-solvers, with C = 8 throughout: eigenvalues within C n eps |A|_2 of the reference (twice that
where the reference is LAPACK float64, n > 32, whose own error has the same bound), residual max|A V - V diag(w)| <= C n eps |A|_2 and
max|V^T V - I| <= C n eps, both formed in long double.  The sweep cap of the Jacobi solvers is 30: a result that needed 30 sweeps stopped on the cap."""
import ctypes as C
import functools

import numpy as np
import pytest

import linalg_ref as R

pytestmark = pytest.mark.gpu

CTOL = 8
EIG_SIZES = [1, 2, 3, 4, 6, 9, 15, 16, 17, 33, 64, 65, 127, 128]
KINDS = ["random", "zero", "diagonal", "repeated", "psd_null", "graded"]


@functools.lru_cache(maxsize=None)
def _matrix(kind, n):
    if kind == "random":
        return R.random_symmetric(n, 1000 + n)
    if kind == "zero":
        return np.zeros((n, n))
    if kind == "diagonal":
        return np.diag(np.random.default_rng(n).standard_normal(n) * 10)
    if kind == "repeated":
        return R.with_spectrum(np.resize([3.0, 3.0, -1.0, 0.5], n), 2000 + n)
    if kind == "psd_null":
        return R.psd_null(n, max(1, (2 * n) // 3), 3000 + n)
    if kind == "graded":
        return R.with_spectrum(np.logspace(-9, 6, n) if n > 1 else [1e6], 4000 + n)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _ref(kind, n):
    A = _matrix(kind, n)
    w, _, src = R.eigh_ref(A)
    return w, src, (float(np.abs(w).max()) if n else 0.0)


def _near_threshold(n, off):
    """Diagonal 1, 1.5, 2, ... with off-diagonal entries `off` on the first super / sub diagonal: every pair starts just above the rotation
    threshold of the Jacobi solvers (1e-15 sqrt|a_pp a_qq|) and every e_i just above QL's convergence test (eps (|d| + |e|)), so a solver that
    stopped early keeps an off-diagonal of size `off` in its residual."""
    A = np.diag(1.0 + 0.5 * np.arange(n))
    for i in range(n - 1):
        A[i, i + 1] = A[i + 1, i] = off
    return A


def _check_eig(A, w, V, wref, src, nrm, what):
    n = A.shape[0]
    tol = CTOL * n * R.EPS * nrm
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V)), what
    err = np.abs(np.sort(w) - wref).max()
    assert err <= (2 * tol if src == "lapack" else tol), (what, "eigenvalues", err, tol)
    res = R.residual(A, w, V)
    assert res <= tol, (what, "residual", res, tol)
    orth = R.orthogonality(V)
    assert orth <= CTOL * n * R.EPS, (what, "orthogonality", orth)


def _jacobi(P, mode, A, nt):
    L = P.lib()
    L.vio_stage_jacobi.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = A.shape[0]
    A = np.ascontiguousarray(A, np.float64)
    w, V, sw = np.zeros(n), np.zeros((n, n)), np.zeros(1, np.int32)
    rc = L.vio_stage_jacobi(mode, n, nt, A.ctypes.data, w.ctypes.data, V.ctypes.data, sw.ctypes.data)
    assert rc == 0, rc
    return w, V, int(sw[0])


def _sym_eig_lds(P, A, one_wave, in_hbm):
    L = P.lib()
    L.vio_stage_sym_eig_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    n = A.shape[0]
    A = np.ascontiguousarray(A, np.float64)
    w, V = np.zeros(n), np.zeros((n, n))
    rc = L.vio_stage_sym_eig_lds(n, one_wave, in_hbm, A.ctypes.data, w.ctypes.data, V.ctypes.data)
    assert rc == 0, rc
    return w, V


# ------------------------------------------------------------------------------------------------------------------------------ Jacobi
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 9, 15, 16])
def test_jacobi_small_and_wave16(P, n):
    """jacobi_small (one thread, be_ingest / be_excalib sizes 3, 4, 6, 9) and jacobi_wave16 (one wavefront of be_marg's 512): accuracy on every kind
    of input, jacobi_wave16 bit for bit equal to jacobi_block (its claim: same pairing, thresholds and rotation order) in LDS and in HBM."""
    for kind in KINDS:
        A = _matrix(kind, n)
        wref, src, nrm = _ref(kind, n)
        w0, V0, _ = _jacobi(P, 0, A, 256)
        _check_eig(A, w0, V0, wref, src, nrm, ("jacobi_small", kind, n))
        w2, V2, s2 = _jacobi(P, 2, A, 512)
        _check_eig(A, w2, V2, wref, src, nrm, ("jacobi_wave16", kind, n))
        assert 1 <= s2 < 30 or (kind == "psd_null" and n >= 15), (kind, n, s2)   # (see test_jacobi_sweep_cap_with_an_exact_null_space)
        if kind in ("zero", "diagonal"):
            assert s2 == 1 and np.array_equal(V2, np.eye(n)) and np.array_equal(w2, np.diag(A)), (kind, n)
            assert np.array_equal(V0, np.eye(n)) and np.array_equal(w0, np.diag(A)), (kind, n)
        for mode in (1, 3):
            wb, Vb, sb = _jacobi(P, mode, A, 512)
            assert sb == s2 and np.array_equal(wb, w2) and np.array_equal(Vb, V2), ("jacobi_block mode", mode, kind, n)


@pytest.mark.parametrize("n", [17, 33, 64, 65, 127, 128])
def test_jacobi_block(P, n):
    """jacobi_block beyond the wavefront sizes (odd n: the round-robin bye), at 512 and 256 threads.  Mode 1 keeps A and V in LDS up to n = 96
    (2 n^2 doubles do not fit 160 KB beyond), so for n <= 96 this compares LDS at 512 threads with HBM at 256 threads bit for bit, and for
    n = 127 and 128 HBM at 512 with HBM at 256."""
    for kind in KINDS:
        A = _matrix(kind, n)
        wref, src, nrm = _ref(kind, n)
        w, V, s = _jacobi(P, 1, A, 512)
        _check_eig(A, w, V, wref, src, nrm, ("jacobi_block", kind, n))
        assert 1 <= s < 30 or (kind == "psd_null" and n >= 15), (kind, n, s)
        if kind in ("zero", "diagonal"):
            assert s == 1 and np.array_equal(V, np.eye(n)) and np.array_equal(w, np.diag(A))
        w3, V3, s3 = _jacobi(P, 3, A, 256)
        assert s3 == s and np.array_equal(w3, w) and np.array_equal(V3, V), (kind, n)


@pytest.mark.xfail(strict=True, reason="known defect (not fixed here: the fix changes the floor, hence the bits of be_marg's fallback): with an exact null space the round-off left between null directions (~eps max|a_ii|) stays "
                   "above the absolute rotation floor 1e-18 max|a_ii|, so jacobi_block / jacobi_wave16 rotate until the 30-sweep cap; the result "
                   "is still accurate (test_jacobi_small_and_wave16)")
def test_jacobi_sweep_cap_with_an_exact_null_space(P):
    """be_marg's Jacobi fallback runs exactly when the 15 x 15 block is (near) singular; it should converge, not stop on the cap."""
    _, _, s = _jacobi(P, 2, _matrix("psd_null", 15), 512)
    assert s < 30, s


@pytest.mark.parametrize("off", [1e-13, 3e-14])
def test_jacobi_rotates_entries_just_above_its_threshold(P, off):
    for n in (2, 3, 6, 16):
        A = _near_threshold(n, off)
        wref, _ = R.mp_eigh(A)
        for mode, nt in ((0, 256), (2, 512), (1, 512)):
            w, V, s = _jacobi(P, mode, A, nt)
            _check_eig(A, w, V, wref, "mpmath", float(np.abs(wref).max()), ("near threshold", mode, n, off))


def test_jacobi_rejects_unsupported_arguments(P):
    L = P.lib()
    L.vio_stage_jacobi.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    A, w, V = np.eye(17), np.zeros(17), np.zeros((17, 17))
    for mode, n, nt in ((0, 17, 256), (2, 17, 512), (4, 4, 512), (1, 0, 512), (1, 257, 512), (1, 4, 100), (1, 4, 2048)):
        assert L.vio_stage_jacobi(mode, n, nt, A.ctypes.data, w.ctypes.data, V.ctypes.data, None) == -1, (mode, n, nt)


# --------------------------------------------------------------------------------------------------------------- Householder + QL
@pytest.mark.parametrize("n", EIG_SIZES)
def test_householder_ql(P, n):
    """sym_eig_tridiag (one wavefront) and sym_eig_tridiag_mt (512 threads), then tridiag_ql_wave, at the call sites of be_prior_factor_kernel
    (LDS with leading dimension n | 1, HBM with n): accuracy on every kind of input, the two address spaces bit for bit equal, and with the
    strict upper triangle full of NaN the decomposition of the lower triangle, bit for bit (the routines read the lower triangle only)."""
    for kind in KINDS:
        A = _matrix(kind, n)
        wref, src, nrm = _ref(kind, n)
        Anan = A.copy()
        Anan[np.triu_indices(n, 1)] = np.nan
        for one_wave in (0, 1):
            w, V = _sym_eig_lds(P, A, one_wave, 0)
            _check_eig(A, w, V, wref, src, nrm, ("householder+ql", one_wave, kind, n))
            wh, Vh = _sym_eig_lds(P, A, one_wave, 1)
            assert np.array_equal(wh, w) and np.array_equal(Vh, V), ("LDS vs HBM", one_wave, kind, n)
            wn, Vn = _sym_eig_lds(P, Anan, one_wave, 0)
            assert np.array_equal(wn, w) and np.array_equal(Vn, V), ("NaN upper triangle", one_wave, kind, n)
            wn, Vn = _sym_eig_lds(P, Anan, one_wave, 1)
            assert np.array_equal(wn, w) and np.array_equal(Vn, V), ("NaN upper triangle, HBM", one_wave, kind, n)


@pytest.mark.parametrize("off", [2e-14, 1e-13])
def test_ql_iterates_on_entries_just_above_its_convergence_test(P, off):
    for n in (2, 3, 6, 16, 65, 128):
        A = _near_threshold(n, off)
        wref, _, src = R.eigh_ref(A)
        for one_wave in (0, 1):
            w, V = _sym_eig_lds(P, A, one_wave, 0)
            _check_eig(A, w, V, wref, src, float(np.abs(wref).max()), ("QL near threshold", one_wave, n, off))


def test_sym_eig_lds_rejects_unsupported_sizes(P):
    L = P.lib()
    L.vio_stage_sym_eig_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    A = np.zeros((129, 129)); w = np.zeros(129); V = np.zeros((129, 129))
    assert L.vio_stage_sym_eig_lds(129, 0, 0, A.ctypes.data, w.ctypes.data, V.ctypes.data) == -1
    assert L.vio_stage_sym_eig_lds(0, 0, 0, A.ctypes.data, w.ctypes.data, V.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------ certified inverse
def _spd_inv(P, A, floor):
    L = P.lib()
    L.vio_stage_spd_inverse16.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    n = A.shape[0]
    A = np.ascontiguousarray(A, np.float64)
    X, ok = np.zeros((n, n)), np.zeros(1, np.int32)
    assert L.vio_stage_spd_inverse16(n, floor, A.ctypes.data, X.ctypes.data, ok.ctypes.data) == 0
    return X, bool(ok[0])


@pytest.mark.parametrize("n", [6, 15, 16])
@pytest.mark.parametrize("floor", [1e-6, 1e-8])
def test_spd_inverse_certificate_sweep(P, n, floor):
    """ok only when the mpmath lambda_min is above floor, and (the rest of the spectrum in [1e-2, 1e2]) whenever it is a factor 1.5 above it; when
    ok, A^-1 within C cond n eps of the mpmath inverse (relative to its largest entry).  lambda_min runs from floor / 1.5^8 to floor * 1.5^8."""
    rng = np.random.default_rng(int(n + 1e3 * (floor == 1e-8)))
    for k in range(-8, 9):
        lmin = floor * 1.5 ** k
        lam = np.concatenate([[lmin], np.exp(rng.uniform(np.log(1e-2), np.log(1e2), n - 1))])
        A = R.with_spectrum(lam, 500 + 17 * n + k)
        lm = R.mp_lambda_min(A)
        X, ok = _spd_inv(P, A, floor)
        if ok:
            # k = 0 puts lambda_min on the floor to within the rounding of A itself: there the certificate can only be right up to the backward
            # error of the factorisation, C n eps |A|_2
            assert lm > floor - (CTOL * n * R.EPS * lam.max() if k == 0 else 0.0), (n, floor, k, float(lm))
            wr, _ = R.mp_eigh(A)
            cond = wr.max() / wr.min()
            Xr = R.mp_inv(A)
            assert np.abs(X - Xr).max() <= CTOL * cond * n * R.EPS * np.abs(Xr).max(), (n, floor, k)
        if k >= 1:
            assert ok, (n, floor, k, float(lm))
        if k < 0:
            assert not ok, (n, floor, k, float(lm))


def test_spd_inverse_certificate_is_strict(P):
    """lambda_min exactly equal to floor is not 'above floor' (1 x 1 and diagonal matrices with powers of two: every step is exact)."""
    X, ok = _spd_inv(P, np.array([[4.0]]), 4.0)
    assert not ok
    X, ok = _spd_inv(P, np.array([[4.0]]), 3.999)
    assert ok and X[0, 0] == 0.25
    X, ok = _spd_inv(P, np.diag([2.0 ** -20, 2.0 ** 10]), 2.0 ** -20)
    assert not ok


@pytest.mark.parametrize("n", [1, 2, 6, 15, 16])
def test_spd_inverse_refuses_bad_input(P, n):
    A = R.with_spectrum(np.linspace(1.0, 3.0, n), 60 + n)
    X, ok = _spd_inv(P, A, 1e-6)
    assert ok
    bad = {"indefinite": R.with_spectrum(np.r_[-1e-3, np.linspace(1.0, 3.0, n - 1)], 61 + n)}
    if n > 1:
        bad["singular"] = R.psd_null(n, n - 1, 62 + n)
    for what, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        B = A.copy(); B[n - 1, n - 1] = v; bad[what + " diagonal"] = B
        if n > 1:
            B = A.copy(); B[n - 1, 0] = B[0, n - 1] = v; bad[what + " off-diagonal"] = B
    for what, B in bad.items():
        X, ok = _spd_inv(P, B, 1e-6)
        assert not ok, (n, what)
    X, ok = _spd_inv(P, np.zeros((n, n)), 1e-6)
    assert not ok


# ---------------------------------------------------------------------------------------------------------- HBM blocked Cholesky
@pytest.mark.parametrize("nb", [1, 4, 11, 12, 21])
@pytest.mark.parametrize("nt", [1024, 512])
def test_blocked_cholesky_against_numpy(P, nb, nt):
    """be_solve's factorisation when the Schur complement does not fit LDS (chol_blocked + chol_solve_blocked, vio_stage_chol blocks = -8 / -9),
    with the assertions of test_tile_cholesky_against_numpy: condition 1e6, the factor to 1e-11 of its largest entry, the solution to 1e-9, NaN
    when a pivot is not positive (the harness returns only the lower triangle, so the zero upper triangle is a property of the harness)."""
    n = 16 * nb
    rng = np.random.default_rng(140 + nb)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (q * np.exp(rng.uniform(0, np.log(1e6), n))) @ q.T
    S = 0.5 * (S + S.T)
    b = rng.standard_normal(n)
    L = np.zeros((n, n)); x = np.zeros(n); us = np.zeros(5)
    blocks = -8 if nt == 1024 else -9
    assert P.lib().vio_stage_chol(nb, 1, blocks, S.ctypes.data, b.ctypes.data, L.ctypes.data, x.ctypes.data, us.ctypes.data) == 0
    Lr = np.linalg.cholesky(S)
    assert np.abs(np.triu(L, 1)).max() == 0.0
    assert np.abs(L - Lr).max() <= 1e-11 * np.abs(Lr).max()
    xr = np.linalg.solve(S, b)
    assert np.abs(x - xr).max() <= 1e-9 * np.abs(xr).max()
    for pos in (0, n // 2, n - 3):
        S2 = S.copy()
        S2[pos, pos] = -1.0
        assert P.lib().vio_stage_chol(nb, 1, blocks, S2.ctypes.data, b.ctypes.data, L.ctypes.data, x.ctypes.data, us.ctypes.data) == 0
        assert np.isnan(x).all(), pos
    if nb == 1:
        assert P.lib().vio_stage_chol(22, 1, blocks, S.ctypes.data, b.ctypes.data, L.ctypes.data, x.ctypes.data, us.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------------ block scan
@pytest.mark.parametrize("nt", [64, 128, 256, 512, 1024])
def test_block_scan_flags(P, nt):
    """Exclusive offsets and total exactly numpy's under every timing skew (thread 0 / the last thread late, flags written by other threads just
    before the call, two scans back to back on the same scratch), the LDS after the scratch untouched."""
    Lb = P.lib()
    Lb.vio_stage_scan_flags.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(nt)
    for n in (0, 1, nt - 1, nt, nt + 1, 7 * nt + 5):
        for pattern in ("random", "zeros", "ones"):
            f = {"random": rng.integers(0, 2, n), "zeros": np.zeros(n), "ones": np.ones(n)}[pattern].astype(np.int32)
            oref, tref = R.exclusive_scan(f)
            for skew in range(16):
                offs = np.full(2 * max(n, 1), -7, np.int32)
                tot = np.zeros(3, np.int32)
                assert Lb.vio_stage_scan_flags(n, nt, skew, f.ctypes.data, offs.ctypes.data, tot.ctypes.data) == 0
                what = (nt, n, pattern, skew)
                assert tot[2] == 1, what
                assert tot[0] == tref and np.array_equal(offs[:n], oref), what
                if skew & 8:
                    assert tot[1] == tref and np.array_equal(offs[n:2 * n], oref), what
    f = np.zeros(4, np.int32)
    assert Lb.vio_stage_scan_flags(4, 96, 0, f.ctypes.data, f.ctypes.data, tot.ctypes.data) == -1
    assert Lb.vio_stage_scan_flags(4, 64, 16, f.ctypes.data, f.ctypes.data, tot.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------------- Schur complement
def _staged_ok(n, nt):   # be_linalg.h schur_staged_ok
    nb = n >> 4
    ntile = nb * (nb + 1) // 2
    return ntile <= 9 * (nt >> 6) and 2 * 16 * (n + 8) + 64 <= ntile * 256 and nb <= 32


def _schur(P, variant, nb, nt, Kpad, colmask, H, Ws, inv, dgp, sp, mu, fill):
    L = P.lib()
    L.vio_stage_schur.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                  C.c_void_p, C.c_void_p]
    n = 16 * nb
    S = np.full((n, n), fill)
    g = np.zeros(1, np.int32)
    Wp = np.ascontiguousarray(Ws if Kpad else np.zeros((1, n)))
    ip = np.ascontiguousarray(inv if Kpad else np.zeros(1))
    rc = L.vio_stage_schur(variant, nb, nt, Kpad, colmask, H.ctypes.data, Wp.ctypes.data, ip.ctypes.data, dgp.ctypes.data, sp.ctypes.data, mu,
                           S.ctypes.data, g.ctypes.data)
    return rc, S, int(g[0])


def _schur_problem(nb, Kpad, mask_kind, seed):
    """A reduced-camera-system-like problem: H symmetric, landmark rows Ws non-zero only in the column tiles of the mask (the pose columns
    0 .. 6 W1 - 1 and the extrinsic / td columns 15 W1 .. 15 W1 + 6 in the real pattern; random gaps otherwise; zero beyond in production too),
    the last Kpad % 7 rows zero (rows >= Fa), a few columns with sp = 0."""
    rng = np.random.default_rng(seed)
    n = 16 * nb
    B = rng.standard_normal((n, n))
    H = np.ascontiguousarray(B @ B.T / n + np.eye(n))
    if mask_kind == "real":
        W1 = max(1, (n - 7) // 15)
        mask = 0
        for cb in range(nb):
            c0, c1 = 16 * cb, 16 * cb + 15
            if c0 < 6 * W1 or (c1 >= 15 * W1 and c0 < 15 * W1 + 7):
                mask |= 1 << cb
    elif mask_kind == "gaps":
        mask = int(sum(1 << cb for cb in range(nb) if cb % 3 != 1)) or 1
    else:
        mask = (1 << nb) - 1
    Ws = rng.standard_normal((Kpad, n))
    for cb in range(nb):
        if not (mask >> cb) & 1:
            Ws[:, 16 * cb:16 * cb + 16] = 0.0
    if Kpad:
        Ws[Kpad - Kpad % 7:] = 0.0
    inv = np.exp(rng.uniform(np.log(1e-2), np.log(1e1), Kpad))
    dgp = np.exp(rng.uniform(np.log(1e-1), np.log(1e1), n))
    sp = np.exp(rng.uniform(np.log(0.3), np.log(3.0), n))
    sp[rng.choice(n, min(3, n), replace=False)] = 0.0
    return H, np.ascontiguousarray(Ws), inv, dgp, sp, mask


def _lower_tiles(nb):
    n = 16 * nb
    ti, tj = np.arange(n)[:, None] // 16, np.arange(n)[None, :] // 16
    return ti >= tj


@pytest.mark.parametrize("nb", [1, 4, 7, 11, 12, 21])
def test_schur_complement(P, nb):
    """schur_mfma, schur_mfma_lds and schur_mfma_staged<9> where be_solve would run them (LDS tiles up to nb = 11, staging where schur_staged_ok;
    nb = 21 is LW = VIO_LWMAX): every lower-tile entry within gamma_(Kpad+6) sum|terms| of the long-double reference, the variants bit for bit
    equal, sp = 0 columns identity rows, tiles outside the staged mask exactly their initial values, the guard words after the tile region intact,
    nothing outside the lower tiles written."""
    n = 16 * nb
    lt = _lower_tiles(nb)
    mu = 0.37
    for Kpad in (0, 4, 16, 20, 252):
        for mask_kind in ("real", "gaps"):
            H, Ws, inv, dgp, sp, mask = _schur_problem(nb, Kpad, mask_kind, 10 * nb + Kpad)
            Sref, bound = R.schur_ref(H, Ws, inv, dgp, sp, mu)
            for nt in (512, 1024):
                variants = [0] + ([1] if nb * (nb + 1) // 2 * 256 <= 16896 else []) + ([2] if nb <= 11 and _staged_ok(n, nt) else [])
                out = {}
                for v in variants:
                    rc, S, g = _schur(P, v, nb, nt, Kpad, mask, H, Ws, inv, dgp, sp, mu, 7.5)
                    what = (nb, Kpad, mask_kind, nt, v)
                    assert rc == 0 and g == 1, (what, rc, g)
                    assert np.all(S[~lt] == 7.5), what
                    err = np.abs(S[lt].astype(np.longdouble) - Sref[lt])
                    assert np.all(err <= bound[lt]), (what, float((err - bound[lt]).max()))
                    z = np.where(sp == 0)[0]
                    for r in z:
                        assert S[r, r] == 1.0 and np.all(S[r, :r][lt[r, :r]] == 0.0) and np.all(S[r + 1:, r][lt[r + 1:, r]] == 0.0), (what, r)
                    out[v] = S
                for v in variants[1:]:
                    assert np.array_equal(out[v], out[0]), (nb, Kpad, mask_kind, nt, "variant", v, "vs schur_mfma")
                if 2 in out:
                    # tiles the mask skips: the scaled H plus mu dgp^2, in the kernel's order of operations
                    S0 = (sp[:, None] * sp[None, :]) * H
                    S0[np.diag_indices(n)] += (mu * dgp) * dgp
                    S0[sp == 0, sp == 0] = 1.0
                    tb = np.arange(n) // 16
                    skip = lt & ~(((mask >> tb[:, None]) & 1) & ((mask >> tb[None, :]) & 1)).astype(bool)
                    assert np.array_equal(out[2][skip], S0[skip]), (nb, Kpad, mask_kind, nt)
            if nb == 1:
                assert not _staged_ok(16, 512) and _schur(P, 2, 1, 512, Kpad, mask, H, Ws, inv, dgp, sp, mu, 0.0)[0] == -1
            if nb >= 12:
                assert _schur(P, 1, nb, 512, Kpad, mask, H, Ws, inv, dgp, sp, mu, 0.0)[0] == -1


# ----------------------------------------------------------------------------------------------------------- truncated pseudo-inverse
def _pinv15(P, A):
    L = P.lib()
    L.vio_stage_pinv15.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    n = A.shape[0]
    A = np.ascontiguousarray(A, np.float64)
    X, path = np.zeros((n, n)), np.zeros(1, np.int32)
    assert L.vio_stage_pinv15(n, A.ctypes.data, X.ctypes.data, path.ctypes.data) == 0
    return X, int(path[0])


@pytest.mark.parametrize("md", [6, 15])
def test_marginalisation_pinv(P, md):
    """be_marg's truncated pseudo-inverse (marg_pinv15, the code be_marg runs) against the mpmath pseudo-inverse with eigenvalues <= 1e-8 dropped,
    for md = 6 (MARGIN_SECOND_NEW) and 15 (MARGIN_OLD), on both sides of the 1e-6 certificate: well inside (certified inverse, path 0), below it
    (Jacobi path 1) with and without eigenvalues under the cut, and an exact null space.  Bound: C cond_kept n eps relative to the largest
    entry, cond_kept = the condition number of the kept spectrum.  The input is not symmetric (the routine symmetrises it)."""
    rng = np.random.default_rng(md)
    cases = {
        "certified": (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), md)), 0),
        "below certificate, nothing dropped": (np.r_[3e-7, np.exp(rng.uniform(np.log(1e-3), np.log(1e3), md - 1))], 1),
        "eigenvalues dropped": (np.r_[1e-10, 2e-9, np.exp(rng.uniform(np.log(1e-3), np.log(1e3), md - 2))], 1),
    }
    for what, (lam, path_expected) in cases.items():
        A = R.with_spectrum(lam, 70 + md)
        skew = rng.standard_normal((md, md)) * 1e-14
        A = A + (skew - skew.T)
        X, path = _pinv15(P, A)
        assert path == path_expected, (md, what, path)
        As = 0.5 * (A + A.T)
        Xr = R.mp_pinv_cut(As, 1e-8)
        wr, _ = R.mp_eigh(As)
        kept = wr[wr > 1e-8]
        tol = CTOL * (kept.max() / kept.min()) * md * R.EPS * np.abs(Xr).max()
        assert np.abs(X - Xr).max() <= tol, (md, what, np.abs(X - Xr).max(), tol)
    G = R.psd_null(md, md - 2, 80 + md)
    X, path = _pinv15(P, G)
    assert path == 1
    Xr = R.mp_pinv_cut(G, 1e-8)
    wr, _ = R.mp_eigh(G)
    kept = wr[wr > 1e-8]
    assert np.abs(X - Xr).max() <= CTOL * (kept.max() / kept.min()) * md * R.EPS * np.abs(Xr).max()
