"""The high-precision references of tests/linalg_ref.py against closed forms, on the CPU: the GPU tests of the be_linalg.h primitives are only as
good as these."""
import mpmath
import numpy as np
import pytest

import linalg_ref as R


@pytest.mark.parametrize("theta", [0.3, 1.0, 2.5])
def test_eigh_of_a_rotated_2x2(theta):
    c, s = np.cos(theta), np.sin(theta)
    Q = np.array([[c, -s], [s, c]])
    A = Q @ np.diag([-1.5, 4.0]) @ Q.T
    A = 0.5 * (A + A.T)
    w, V = R.mp_eigh(A)
    assert np.abs(w - [-1.5, 4.0]).max() <= 8 * R.EPS * 4.0
    assert abs(abs(V[:, 1] @ Q[:, 1]) - 1.0) <= 8 * R.EPS
    assert R.residual(A, w, V) <= 8 * R.EPS * 4.0
    assert R.orthogonality(V) <= 4 * R.EPS


def test_eigh_of_diagonal_and_zero_matrices():
    d = np.array([3.0, -2.0, 0.0, 7.5, 1e-9])
    w, V = R.mp_eigh(np.diag(d))
    assert np.array_equal(w, np.sort(d))
    assert np.array_equal(np.abs(V), np.eye(5)[:, np.argsort(d)])
    w, V = R.mp_eigh(np.zeros((4, 4)))
    assert np.array_equal(w, np.zeros(4)) and R.orthogonality(V) == 0.0


def test_eigh_with_a_known_spectrum_and_lapack_agree():
    lam = np.array([1e-9, 1e-3, 1.0, 2.0, 2.0, 1e6])
    A = R.with_spectrum(lam, 1)
    w, V, src = R.eigh_ref(A)
    assert src == "mpmath"
    assert np.abs(w - lam).max() <= 16 * R.EPS * 1e6           # A itself carries the round-off of Q diag(lam) Q^T
    assert R.residual(A, w, V) <= 4 * R.EPS * 1e6               # but the reference decomposes the rounded A exactly
    assert np.abs(w - np.linalg.eigvalsh(A)).max() <= 16 * R.EPS * 1e6
    assert R.eigh_ref(R.random_symmetric(40, 2))[2] == "lapack"


def test_inverse_pinv_and_lambda_min_closed_forms():
    A = np.array([[4.0, 2.0], [2.0, 3.0]])                      # inverse [[3, -2], [-2, 4]] / 8
    assert np.abs(R.mp_inv(A) - np.array([[3.0, -2.0], [-2.0, 4.0]]) / 8).max() <= R.EPS
    lm = R.mp_lambda_min(A)                                     # (7 - sqrt 17) / 2
    with mpmath.workdps(40):
        assert abs(lm - (7 - mpmath.sqrt(17)) / 2) < mpmath.mpf(10) ** -35
    assert R.mp_lambda_min(np.diag([5.0, 1e-6, 2.0])) == mpmath.mpf(1e-6)
    P = R.mp_pinv_cut(np.diag([2.0, 1e-9, 4.0, 0.0]), 1e-8)
    assert np.array_equal(P, np.diag([0.5, 0.0, 0.25, 0.0]))
    G = R.psd_null(6, 4, 3)
    assert np.array_equal(G[4], G[0]) and np.array_equal(G[:, 5], G[:, 1])
    w, _ = R.mp_eigh(G)
    assert np.abs(w[:2]).max() <= 1e-30 + 0.0 and w[2] > 1e-3


def test_cholesky_reference():
    A = np.array([[4.0, 2.0, -2.0], [2.0, 10.0, 2.0], [-2.0, 2.0, 6.0]])   # L = [[2, 0, 0], [1, 3, 0], [-1, 1, 2]]
    assert np.array_equal(R.mp_cholesky(A), np.array([[2.0, 0, 0], [1.0, 3.0, 0], [-1.0, 1.0, 2.0]]))
    A[2, 2] = 1.0
    assert R.mp_cholesky(A) is None


def test_exclusive_scan():
    o, t = R.exclusive_scan([1, 0, 1, 1, 0])
    assert list(o) == [0, 1, 1, 2, 3] and t == 3
    o, t = R.exclusive_scan([])
    assert len(o) == 0 and t == 0
